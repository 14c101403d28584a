"""CPU: the DPM-Solver++ multistep sampler.  The library's host-only coefficient table against the float64 restatement, order 1
against DDIM, exactness on a constant x0-prediction, convergence on an analytic Gaussian score, and DPMSolverSampler's plumbing on
host stand-in models."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dpm_solver_ref as dref
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler, dpmpp_coefficients
from makeupdiffuse_amd.engine import dpmpp_table
from oracle import sampler

S_ALL = (5, 9, 10, 20, 50)


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
        self.calls = []

    def apply_model(self, x, t, c):
        self.calls.append((tuple(x.shape), int(t[0]), c))
        return self.eps_fn(x, t, c)


def alpha_of(t):
    """alphas_cumprod (the fp32 buffer, as a float64 number) at integer timesteps t [B]"""
    return sampler.Schedule().alphas_cumprod.double()[t].view(-1, *([1] * 3))


# ---- 1. the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('lof', [True, False])
def test_table_equals_the_restatement(S, order, lof):
    _, a, ap = dref.grid(S)
    coef, so = dpmpp_table(a, ap, order, lof)
    ref, ref_orders = dref.coefficients(a, ap, order, lof)
    assert coef.dtype == np.float32 and coef.shape == (S, 6)
    ref32 = ref.astype(np.float32).astype(np.float64)
    err = np.abs(coef.astype(np.float64) - ref32)
    assert (err <= 1e-6 * np.abs(ref32)).all(), f'S {S} order {order}: max rel {np.max(err / np.maximum(np.abs(ref32), 1e-300)):.3e}'
    assert so.tolist() == ref_orders.tolist()
    # the rule, written out: entry i is executed step k = S - 1 - i
    for i in range(S):
        k = S - 1 - i
        want = min(order, k + 1)
        if lof and S < 10:
            want = min(want, S - k)
        assert so[i] == want
        assert (coef[i, 4] != 0) == (want >= 2) and (coef[i, 5] != 0) == (want >= 3)
    # the Python double form the host path uses is the same table
    py, py_orders = dpmpp_coefficients(a, ap, order, lof)
    assert np.allclose(py, ref, rtol=1e-11, atol=0) and py_orders.tolist() == ref_orders.tolist()


def test_final_step_orders_of_order_three():
    for S, last_two in ((9, [2, 1]), (10, [3, 3])):
        _, a, ap = dref.grid(S)
        _, so = dpmpp_table(a, ap, 3, True)
        assert [int(so[1]), int(so[0])] == last_two, (S, so)
    _, a, ap = dref.grid(9)
    _, so = dpmpp_table(a, ap, 3, False)
    assert [int(so[1]), int(so[0])] == [3, 3]


def test_table_bad_arguments_need_no_device():
    lib = mlib.load()
    _, a, ap = dref.grid(10)
    n = len(a)
    out = (ctypes.c_float * (6 * n))()
    fa = lambda v: (ctypes.c_float * len(v))(*[float(x) for x in v])
    assert lib.mkd_dpmpp_table(n, fa(a), fa(ap), 2, 1, out, None) == 0                     # step_order may be NULL
    for order in (0, 4, -1):
        assert lib.mkd_dpmpp_table(n, fa(a), fa(ap), order, 1, out, None) == -1            # MKD_ERR_ARG
    assert lib.mkd_dpmpp_table(n, fa(ap), fa(a), 2, 1, out, None) == -1                    # lambda decreases within a step (inversion tables)
    assert lib.mkd_dpmpp_table(n, fa(a[::-1]), fa(ap[::-1]), 2, 1, out, None) == -1        # ... along the loop
    bad_prev = list(ap); bad_prev[0] = 1.0
    assert lib.mkd_dpmpp_table(n, fa(a), fa(bad_prev), 2, 1, out, None) == -1              # a >= 1
    bad = list(a); bad[-1] = 0.0
    assert lib.mkd_dpmpp_table(n, fa(bad), fa(ap), 2, 1, out, None) == -1
    assert lib.mkd_dpmpp_table(0, fa(a), fa(ap), 2, 1, out, None) == -1
    with pytest.raises(mlib.MkdError):
        dpmpp_table(a, ap, 5)
    with pytest.raises(ValueError):
        dpmpp_coefficients(a, ap, 5)
    with pytest.raises(ValueError):
        dpmpp_coefficients(ap, a, 2)


# ---- 2. order 1 is DDIM ------------------------------------------------------------------------------------------------------
class DDIMSampler64(DDIMSampler):
    """DDIMSampler with its one derived table at the precision of the comparison: make_schedule registers
    ddim_sqrt_one_minus_alphas = sqrt(1 - a) rounded to float32 (as upstream does) while its update takes sqrt(a_t) and sqrt(1 - a_prev)
    of the same alphas in double, so the stock class carries a 2^-24 relative table rounding (~6e-8) that no float64 solver on the
    same alphas can reproduce.  Here that table is sqrt(1 - float64(ddim_alphas)); loop, batching and update are DDIMSampler's."""

    def make_schedule(self, *a, **kw):
        super().make_schedule(*a, **kw)
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - self.ddim_alphas.double())


@pytest.mark.parametrize('S', [5, 10, 20])
@pytest.mark.parametrize('cfg', [False, True])
def test_order_one_equals_ddim_in_fp64(S, cfg):
    """Order 1 against DDIMSampler (eta 0), same grid, float64 stand-in model: <= 1e-12 once DDIMSampler's sqrt(1 - a) table is
    float64 too (DDIMSampler64).  Against the stock class the distance is its own float32 table rounding: measured 5.7e-8 (S 5) and
    below, bounded here by S x 2^-23 x max |eps| (one table rounding per step, amplified by at most 1 / alpha_t x alpha_prev < 2)."""
    def eps(x, t, c):
        return torch.tanh(0.7 * x + c['shift']) * (1.0 + 1e-3 * t.view(-1, 1, 1, 1).double())
    m = HostModel(eps)
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(2, 4, 5, 5, generator=g, dtype=torch.float64)
    c = {'shift': torch.randn(2, 1, 1, 1, generator=g, dtype=torch.float64)}
    uc = {'shift': torch.randn(2, 1, 1, 1, generator=g, dtype=torch.float64)} if cfg else None
    kw = dict(conditioning=c, x_T=x_T, unconditional_guidance_scale=4.0 if cfg else 1.0, unconditional_conditioning=uc)
    ddim, _ = DDIMSampler64(m).sample(S, 2, (4, 5, 5), eta=0.0, verbose=False, **kw)
    stock, _ = DDIMSampler(m).sample(S, 2, (4, 5, 5), eta=0.0, verbose=False, **kw)
    dpm, _ = DPMSolverSampler(m).sample(S, 2, (4, 5, 5), order=1, **kw)
    assert dpm.dtype == torch.float64
    d, d_stock = (dpm - ddim).abs().max().item(), (dpm - stock).abs().max().item()
    print(f'[dpm] order 1 vs DDIM, S {S}, cfg {cfg}: max |delta| {d:.3e} (stock float32 sqrt(1 - a) table: {d_stock:.3e})')
    assert d <= 1e-12
    assert d_stock <= S * 2 ** -23 * (2.0 * (4.0 + 3.0 if cfg else 1.0))          # |eps| <= 2, guidance 4: |e| <= 2 (1 + 2 * 3)
    two, _ = DPMSolverSampler(m).sample(S, 2, (4, 5, 5), order=2, **kw)
    assert (two - ddim).abs().max().item() > 1e-6                # order 2 is another map (not a vacuous equality)


# ---- 3. exactness on a constant x0-prediction ---------------------------------------------------------------------------------
@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('order', [1, 2, 3])
def test_constant_x0_prediction_is_integrated_exactly(S, order):
    g = torch.Generator().manual_seed(5)
    cst = torch.randn(1, 4, 3, 3, generator=g, dtype=torch.float64)
    x_T = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)

    def eps(x, t, c):
        a = alpha_of(t)
        return (x - a.sqrt() * cst) / (1.0 - a).sqrt()
    ts, a, ap = dref.grid(S)
    a_T, a_0 = float(a[-1]), float(ap[0])
    exact = math.sqrt(a_0) * cst + math.sqrt((1.0 - a_0) / (1.0 - a_T)) * (x_T - math.sqrt(a_T) * cst)
    ref = dref.dpm_solver_pp(eps, ts, a, ap, x_T, order=order)
    assert (ref - exact).abs().max().item() <= 1e-12, 'restatement'
    if 1000 % S:
        return                                               # (S = 9: make_schedule's uniform grid has no 9-entry form; the class runs the other S)
    for lof in (True, False):
        out, _ = DPMSolverSampler(HostModel(eps)).sample(S, 2, (4, 3, 3), x_T=x_T, order=order, lower_order_final=lof)
        d = (out - exact).abs().max().item()
        assert d <= 1e-12, f'S {S} order {order}: {d:.3e}'


# ---- 4. convergence on an analytic score ----------------------------------------------------------------------------------------
GAUSS = ((0.7, 0.5), (0.0, 0.2), (-1.0, 1.5))
S_CONV = (5, 8, 10, 20, 25, 50)


def gauss_errors(mu, s, run):
    """max |x_0 - exact| of run(eps, S, order) for data N(mu, s^2 I): eps*(x, a) = sigma (x - alpha mu) / (a s^2 + 1 - a)"""
    x_T = torch.tensor(np.random.default_rng(0).standard_normal(4096), dtype=torch.float64).view(1, 4, 32, 32)

    def eps(x, t, c):
        a = alpha_of(t)
        return (1.0 - a).sqrt() * (x - a.sqrt() * mu) / (a * s * s + 1.0 - a)
    v = lambda a: a * s * s + 1.0 - a
    out = {}
    for S in S_CONV:
        _, a, ap = dref.grid(S)
        a_T, a_0 = float(a[-1]), float(ap[0])
        exact = math.sqrt(a_0) * mu + math.sqrt(v(a_0) / v(a_T)) * (x_T - math.sqrt(a_T) * mu)
        for order in (1, 2):
            out[S, order] = (run(eps, S, order, x_T) - exact).abs().max().item()
    return out


@pytest.mark.parametrize('which', ['restatement', 'sampler'])
def test_order_two_converges_faster_on_a_gaussian(which):
    if which == 'restatement':
        def run(eps, S, order, x_T):
            ts, a, ap = dref.grid(S)
            return dref.dpm_solver_pp(eps, ts, a, ap, x_T, order=order)
    else:
        def run(eps, S, order, x_T):
            return DPMSolverSampler(HostModel(eps)).sample(S, 1, (4, 32, 32), x_T=x_T, order=order)[0]
    for mu, s in GAUSS:
        err = gauss_errors(mu, s, run)
        print(f'[dpm] {which} N({mu}, {s}^2): ' + ', '.join(f'S {S}: o1 {err[S, 1]:.3e} o2 {err[S, 2]:.3e}' for S in S_CONV))
        for S in S_CONV:
            assert err[S, 2] < err[S, 1], f'N({mu}, {s}^2) S {S}: order 2 {err[S, 2]:.3e} !< order 1 {err[S, 1]:.3e}'
        if (mu, s) == (-1.0, 1.5):
            assert err[25, 2] < err[50, 1], f'order 2 at 25 steps {err[25, 2]:.3e} !< DDIM at 50 {err[50, 1]:.3e}'


def test_ddim_sampler_has_the_order_one_error_on_the_gaussian():
    """the order-1 column above IS DDIM: DDIMSampler itself at 50 steps, against DPM-Solver++ order 2 at 25"""
    mu, s = GAUSS[2]

    def run(eps, S, order, x_T):
        m = HostModel(eps)
        if order == 1:
            return DDIMSampler(m).sample(S, 1, (4, 32, 32), x_T=x_T, eta=0.0, verbose=False)[0]
        return DPMSolverSampler(m).sample(S, 1, (4, 32, 32), x_T=x_T, order=2)[0]
    err = gauss_errors(mu, s, run)
    assert err[25, 2] < err[50, 1]


# ---- 5. plumbing ----------------------------------------------------------------------------------------------------------------
def test_unconditional_first_batching_and_callback_count():
    m = HostModel(lambda x, t, c: 0.1 * x + c['v'])
    S, B = 5, 2
    x_T = torch.randn(B, 4, 3, 3)
    c = {'v': torch.full((B, 1, 1, 1), 2.0)}
    uc = {'v': torch.full((B, 1, 1, 1), -1.0)}
    seen = []
    out, inter = DPMSolverSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, unconditional_guidance_scale=3.0,
                                            unconditional_conditioning=uc, callback=seen.append)
    assert seen == list(range(S))
    assert len(m.calls) == S and all(shape[0] == 2 * B for shape, _, _ in m.calls)
    assert torch.equal(m.calls[0][2]['v'][:B], uc['v']) and torch.equal(m.calls[0][2]['v'][B:], c['v'])      # unconditional FIRST
    steps = [t for _, t, _ in m.calls]
    assert steps == [int(t) for t in np.flip(sampler.Schedule().make_ddim(S).ddim_timesteps)]
    assert inter['x_inter'][0] is x_T and inter['x_inter'][-1] is out
    ts, a, ap = dref.grid(S)
    # guidance combine e_u + s (e_c - e_u), checked against the restatement driven with the combined eps
    comb = dref.dpm_solver_pp(lambda x, t, cc: (0.1 * x - 1.0) + 3.0 * ((0.1 * x + 2.0) - (0.1 * x - 1.0)), ts, a, ap, x_T.double())
    torch.testing.assert_close(out.double(), comb, rtol=1e-5, atol=1e-5)
    # without guidance: one un-doubled evaluation per step
    m.calls.clear()
    DPMSolverSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T)
    assert len(m.calls) == S and all(shape[0] == B for shape, _, _ in m.calls)


def test_fast_hook_gets_the_tables_and_the_blend_draws():
    m = HostModel(lambda x, t, c: 0.1 * x)
    S, B = 5, 2
    x_T, x0 = torch.randn(B, 4, 3, 3), torch.randn(B, 4, 3, 3)
    mask = torch.ones(B, 1, 3, 3)
    seen = {}

    def fast(x, c, timesteps, alphas, alphas_prev, order, lower_order_final, scale=1.0, uc=None, **kw):
        seen.update(kw, timesteps=list(timesteps), alphas=list(alphas), alphas_prev=list(alphas_prev), order=order, lof=lower_order_final)
        return x
    m.sample_loop_dpmpp = fast
    torch.manual_seed(9)
    out, _ = DPMSolverSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, order=3, lower_order_final=False, mask=mask, x0=x0)
    assert out is x_T
    sch = sampler.Schedule().make_ddim(S)
    assert seen['timesteps'] == list(sch.ddim_timesteps) and seen['order'] == 3 and seen['lof'] is False
    assert np.allclose(seen['alphas'], sch.ddim_alphas.numpy()) and np.allclose(seen['alphas_prev'], sch.ddim_alphas_prev.numpy())
    torch.manual_seed(9)
    draws = torch.stack([torch.randn_like(x0) for _ in range(S)])
    assert torch.equal(seen['q_noise'], draws)
    assert np.allclose(seen['q_sqrt_ac'], [float(m.sqrt_alphas_cumprod[t]) for t in sch.ddim_timesteps])
    assert np.allclose(seen['q_sqrt_1m_ac'], [float(m.sqrt_one_minus_alphas_cumprod[t]) for t in sch.ddim_timesteps])
    # a callback takes the per-step loop instead
    seen.clear()
    DPMSolverSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, callback=lambda k: None)
    assert not seen


def test_masked_step_loop_equals_the_restatement():
    eps = lambda x, t, c: 0.3 * torch.tanh(x)
    m = HostModel(eps)
    S, B = 5, 2
    g = torch.Generator().manual_seed(12)
    x_T, x0 = torch.randn(B, 4, 3, 3, generator=g), torch.randn(B, 4, 3, 3, generator=g)
    mask = (torch.rand(B, 1, 3, 3, generator=g) > 0.5).float()
    torch.manual_seed(21)
    out, _ = DPMSolverSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, mask=mask, x0=x0)
    torch.manual_seed(21)
    draws = [torch.randn_like(x0) for _ in range(S)]
    ts, a, ap = dref.grid(S)

    def blend(k, step, img):
        q = float(m.sqrt_alphas_cumprod[step]) * x0 + float(m.sqrt_one_minus_alphas_cumprod[step]) * draws[k]
        return q * mask + (1.0 - mask) * img
    ref = dref.dpm_solver_pp(eps, ts, a, ap, x_T, blend=blend)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    plain, _ = DPMSolverSampler(m).sample(S, B, (4, 3, 3), x_T=x_T)
    assert (out - plain).abs().max() > 1e-3


def test_rejected_options_and_mask_errors():
    m = HostModel(lambda x, t, c: 0.1 * x)
    s = DPMSolverSampler(m)
    x_T = torch.randn(2, 4, 3, 3)
    for kw in (dict(eta=0.5), dict(score_corrector=object()), dict(dynamic_threshold=0.9), dict(corrector_kwargs={'a': 1}),
               dict(ucg_schedule=[1.0]), dict(quantize_x0=True), dict(temperature=0.5), dict(noise_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            s.sample(4, 2, (4, 3, 3), x_T=x_T, **kw)
    s.sample(4, 2, (4, 3, 3), x_T=x_T, eta=0.0, verbose=False)             # the call shape log_results uses
    with pytest.raises(ValueError):
        s.sample(4, 2, (4, 3, 3), x_T=x_T, order=4)
    # mask shape errors are DDIMSampler's (_check_mask)
    ddim = DDIMSampler(m)
    for mask, x0 in ((torch.ones(2, 1, 3, 3), None), (torch.ones(3, 1, 3, 3), torch.zeros(2, 4, 3, 3)),
                     (torch.ones(2, 2, 3, 3), torch.zeros(2, 4, 3, 3)), (torch.ones(2, 1, 3, 3), torch.zeros(2, 4, 3, 2))):
        with pytest.raises(ValueError) as e1:
            s.sample(4, 2, (4, 3, 3), x_T=x_T, mask=mask, x0=x0)
        with pytest.raises(ValueError) as e2:
            ddim.sample(4, 2, (4, 3, 3), x_T=x_T, mask=mask, x0=x0, verbose=False)
        assert str(e1.value) == str(e2.value)


def test_decode_uses_the_first_t_start_entries():
    eps = lambda x, t, c: 0.2 * x
    m = HostModel(eps)
    s = DPMSolverSampler(m)
    s.make_schedule(10)
    x = torch.randn(1, 4, 3, 3, dtype=torch.float64)
    sch = sampler.Schedule().make_ddim(10)
    for t_start, order in ((4, 2), (7, 3), (10, 2), (1, 2)):
        m.calls.clear()
        out = s.decode(x, None, t_start, order=order)
        assert [t for _, t, _ in m.calls] == [int(t) for t in np.flip(sch.ddim_timesteps[:t_start])]
        ref = dref.dpm_solver_pp(eps, sch.ddim_timesteps[:t_start], sch.ddim_alphas[:t_start].numpy(), sch.ddim_alphas_prev[:t_start].numpy(),
                                 x, order=order)
        assert (out - ref).abs().max().item() <= 1e-12
    assert s.decode(x, None, 0) is x
    with pytest.raises(ValueError):
        s.decode(x, None, 11)
    # a latent inverted with DDIMSampler.encode comes back (x-independent eps: the inversion is exact for order 1)
    flat = HostModel(lambda xx, t, c: torch.full_like(xx, 0.3))
    d = DDIMSampler(flat); d.make_schedule(10, verbose=False)
    enc, _ = d.encode(x, None, 6)
    sd = DPMSolverSampler(flat); sd.make_schedule(10)
    assert (sd.decode(enc, None, 6, order=1) - x).abs().max().item() <= 1e-6
