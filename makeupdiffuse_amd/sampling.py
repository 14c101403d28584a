"""The samplers' loop driver (host logic): one record per solver and, once each, the parts every sampler class is built from -- the
start latent, the masked blend's keywords, the fast path (the whole loop inside libmkd through a model hook, with its trace merged into
the intermediates), the step loop (blend, step, callback, trace) and the host guided eps.  ``ddim.DDIMSampler`` runs its loops on it;
``dpm_solver.DPMSolverSampler`` and ``unipc.UniPCSampler`` are ``MultistepSampler`` with their record.  ``MkdEngine`` and the model
read the same records for the exported entries and the hook names."""
from __future__ import annotations

import importlib
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

__all__ = ['Solver', 'SOLVERS', 'MultistepSampler']


def _later(module, name):
    """a function of a sibling module, imported at its first call (the solver modules import this one; engine loads libmkd)"""
    return lambda *args: getattr(importlib.import_module(module, __package__), name)(*args)


def _ddim_update(x, e_t, c, noise=None, temperature=1.0):
    a_t, a_prev, sigma_t, s1m_t = c
    pred_x0 = (x - s1m_t * e_t) / a_t ** 0.5
    dir_xt = (1.0 - a_prev - sigma_t ** 2) ** 0.5 * e_t
    x_prev = a_prev ** 0.5 * pred_x0 + dir_xt
    if noise is not None:
        x_prev = x_prev + sigma_t * noise * temperature
    return x_prev, pred_x0


def _dpmpp_update(x, e_t, c, m1, m2):
    inv_alpha, sigma, cx, c0, c1, c2 = c
    m0 = (x - sigma * e_t) * inv_alpha
    x = cx * x + c0 * m0
    if c1 != 0.0:
        x = x + c1 * m1
    if c2 != 0.0:
        x = x + c2 * m2
    return x, m0


def _unipc_update(x, xc, e_t, c, *hist):
    m0 = (x - c[1] * e_t) * c[0]
    if c[2] != 0.0:
        xc = c[2] * xc + c[3] * m0
        for cj, mj in zip(c[4:7], hist):
            if cj != 0.0:
                xc = xc + cj * mj
    else:
        xc = x
    x = c[7] * xc + c[8] * m0
    for cj, mj in zip(c[9:11], hist):
        if cj != 0.0:
            x = x + cj * mj
    return x, xc, m0


@dataclass(frozen=True)
class Solver:
    name: str                          # TestDiffuseModel.sampler, batching.build_rows
    title: str                         # in messages
    rows_id: Optional[int]             # the id mkd_sample_rows takes; None: the per-sample loop does not run this solver
    masked: bool                       # takes mask / x0
    loop_hook: str                     # model hook: the whole loop inside libmkd
    loop: str                          # MkdEngine's method behind it; the exported entries are mkd_<loop>[_ex]
    step: str                          # model hook and MkdEngine method of one update; exported as mkd_<step>[_ex]
    options: Tuple[Tuple[str, str], ...] = ()   # (sampler keyword, model attribute) of the solver's own options
    # one update is step(x, *carried, e_c, e_u, scale, coefficient row, *history) -> (next latent, *carried, x0-prediction)
    depth: int = 0                     # x0-predictions of earlier steps in the history
    carried: int = 0                   # latents carried beside x (UniPC's corrected one)
    host_table: Optional[Callable] = None      # float64 coefficient rows, and the floats of libmkd's table for the step kernel
    device_table: Optional[Callable] = None
    host_update: Optional[Callable] = None     # the update in torch, with the guided eps in place of (e_c, e_u, scale)


SOLVERS = {s.name: s for s in (
    # (DDIM's row is the step's a_t, a_prev, sigma_t, sqrt(1 - a_t), straight from the schedule: no table)
    Solver('ddim', 'DDIM', rows_id=0, masked=True, loop_hook='sample_loop_fast', loop='sample', step='ddim_step',
           host_update=_ddim_update),
    Solver('dpmpp', 'DPM-Solver++', rows_id=1, masked=True, loop_hook='sample_loop_dpmpp', loop='sample_dpmpp', step='dpmpp_step',
           options=(('order', 'solver_order'),), depth=2, host_table=_later('.dpm_solver', 'dpmpp_coefficients'),
           device_table=_later('.engine', 'dpmpp_table'), host_update=_dpmpp_update),
    Solver('unipc', 'UniPC', rows_id=None, masked=False, loop_hook='sample_loop_unipc', loop='sample_unipc', step='unipc_step',
           options=(('order', 'solver_order'), ('corrector', 'unipc_corrector')), depth=3, carried=1,
           host_table=_later('.unipc', 'unipc_coefficients'), device_table=_later('.engine', 'unipc_table'), host_update=_unipc_update))}


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def rescale_guided_eps(e_c, e_u, scale, phi):
    """The guided eps with guidance rescale, in torch (host tensors; the device path is mkd_cfg_rescale_factor + the step kernels):
    g = e_u + scale (e_c - e_u), per sample k = phi std(e_c) / std(g) + (1 - phi) (std(g) == 0: 1), returns g k."""
    g = guided_eps(e_c, e_u, scale)
    dims = tuple(range(1, g.dim()))
    s_c, s_g = e_c.std(dim=dims, keepdim=True), g.std(dim=dims, keepdim=True)
    k = torch.where(s_g > 0, phi * s_c / torch.where(s_g > 0, s_g, torch.ones_like(s_g)) + (1.0 - phi), torch.ones_like(s_g))
    return g * k


def guided_eps(e_c, e_u, scale, phi=0.0):
    """the eps of a host update: e_c without an unconditional half, else e_u + scale (e_c - e_u), rescaled where phi is engaged"""
    if e_u is None:
        return e_c
    if phi != 0.0:
        return rescale_guided_eps(e_c, e_u, scale, phi)
    return e_u + scale * (e_c - e_u)


def start_latent(size, x_T, seeds, device):
    """the start latent: x_T as given, else noise.normal on stream 0 with seeds, else a torch draw"""
    if x_T is not None:
        return x_T
    if seeds is not None:
        from .noise import STREAM_START, normal
        return normal(seeds, tuple(size)[1:], stream=STREAM_START, device=device)
    return torch.randn(size, device=device)


def blend_kwargs(q_tables, x0, mask, timesteps, seeds=None, draws=None):
    """the masked blend's keywords of a loop hook: the DDPM tables at each entry's timestep and the blend's noise, one row per executed
    step -- with seeds rows 0 .. n - 1 of stream 2 in one launch, else ``draws`` (the randn_like(x0) the caller took in loop order among
    its other draws) or n draws taken here"""
    n = len(timesteps)
    if seeds is not None:
        from .noise import STREAM_BLEND, normal
        q_noise = normal(seeds, tuple(x0.shape)[1:], stream=STREAM_BLEND, rows=n, device=x0.device)
    else:
        q_noise = torch.stack(draws if draws is not None else [torch.randn_like(x0) for _ in range(n)])
    sa, s1 = q_tables
    return dict(x0=x0, mask=mask, q_sqrt_ac=[float(sa[int(t)]) for t in timesteps], q_sqrt_1m_ac=[float(s1[int(t)]) for t in timesteps],
                q_noise=q_noise)


def merge_trace(res, trace):
    """a loop hook's result -> the latent.  (latent, x_inter rows, pred_x0 rows) is appended to the intermediates of ``trace`` =
    (log_every_t, the dict); the latent stays the last x_inter entry.  A hook that keeps no trace returns the latent alone."""
    if not isinstance(res, tuple):
        return res
    img, x_rows, x0_rows = res
    trace[1]['x_inter'] += [*x_rows[:-1], img]
    trace[1]['pred_x0'] += list(x0_rows)
    return img


def fast_loop(hook, img, cond, tables, scale, uc, kw=(), trace=None, phi=0.0):
    """the whole loop inside libmkd: ``hook(img, cond, *tables, scale, uc, **kw)`` with the trace and the engaged rescale asked for"""
    kw = dict(kw)
    if trace is not None:
        kw['log_every_t'] = int(trace[0])
    if phi != 0.0:
        kw['guidance_rescale'] = phi
    return merge_trace(hook(img, cond, *tables, scale, uc, **kw), trace)


def step_loop(img, timesteps, step, callback=None, blend=None, trace=None, forward=False):
    """the loop over the table entries, step by step: executed step k is entry n - 1 - k (``forward``: entry k, the inversion's order).
    ``blend(t, img, k)`` before the step, ``step(img, ts, index, k) -> (img, x0-prediction)``, ``callback(k)``, then the trace's rows:
    the entries with index % log_every_t == 0 and the first executed one"""
    n = len(timesteps)
    for k in range(n):
        index = k if forward else n - 1 - k
        t = int(timesteps[index])
        if blend is not None:
            img = blend(t, img, k)
        img, pred_x0 = step(img, torch.full((img.shape[0],), t, device=img.device, dtype=torch.long), index, k)
        if callback:
            callback(k)
        if trace is not None and (index % trace[0] == 0 or index == n - 1):
            trace[1]['x_inter'].append(img)
            trace[1]['pred_x0'].append(pred_x0)
    return img


class MultistepSampler:
    """A deterministic multistep solver on the step grid and tables of ``DDIMSampler.make_schedule(S)``; ``solver`` is its record."""
    solver: Solver
    # options of upstream samplers that these deterministic solvers do not have
    _REJECTED = ('score_corrector', 'corrector_kwargs', 'dynamic_threshold', 'ucg_schedule', 'img_callback', 'quantize_x0')

    def __init__(self, model, **kwargs):
        from .ddim import DDIMSampler
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self._ddim = DDIMSampler(model)          # the step grid, its tables, the guidance batching and the masked blend

    def make_schedule(self, num_steps, verbose=False):
        """The grid of DDIMSampler.make_schedule(num_steps): ddim_timesteps / ddim_alphas / ddim_alphas_prev."""
        self._ddim.make_schedule(ddim_num_steps=num_steps, ddim_eta=0.0, verbose=verbose)
        self.ddim_timesteps = self._ddim.ddim_timesteps
        self.ddim_alphas = self._ddim.ddim_alphas
        self.ddim_alphas_prev = self._ddim.ddim_alphas_prev

    # sample() of the two classes; args = (order, lower_order_final[, corrector]), what the hook and the tables take after the grid
    def _sample(self, S, batch_size, shape, cond, x_T, scale, uc, args, callback, mask, x0, log_every_t, guidance_rescale, seeds, kw):
        from .ddim import _check_mask, _check_rescale, _check_seeds
        name, title = type(self).__name__, self.solver.title
        if kw.get('eta') not in (None, 0, 0.0):
            raise NotImplementedError(f'{name} is deterministic: eta is not an option of {title}')
        for k in self._REJECTED:
            if kw.get(k) not in (None, False):
                raise NotImplementedError(f'{name}.sample option {k} is not on the MakeupDiffuse path')
        if kw.get('temperature', 1.0) != 1.0 or kw.get('noise_dropout', 0.0) != 0.0:
            raise NotImplementedError(f'{name} draws no noise: temperature / noise_dropout do not apply')
        if not self.solver.masked and (mask is not None or x0 is not None):
            raise NotImplementedError(f'{name}: masked sampling (mask / x0) is not defined for this solver: the blend would have '
                                      'to act on the two latents it carries')
        if args[0] not in (1, 2, 3):
            raise ValueError(f'{name}: order must be 1, 2 or 3')
        C, H, W = shape
        size = (batch_size, C, H, W)
        _check_mask(mask, x0, size)
        phi = _check_rescale(guidance_rescale)
        if uc is None or scale == 1.0:
            phi = 0.0          # no unconditional half: not engaged
        if int(log_every_t) < 1:
            raise ValueError(f'log_every_t must be >= 1, got {log_every_t}')
        if seeds is not None:
            seeds = _check_seeds(seeds, batch_size)
        self.make_schedule(S, verbose=False)
        img = start_latent(size, x_T, seeds, self.model.device)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        img = self._run(img, cond, len(self.ddim_timesteps), scale, uc, args, callback, mask, x0, (int(log_every_t), intermediates), phi,
                         seeds)
        if len(intermediates['x_inter']) == 1:          # (a hook that keeps no trace)
            intermediates['x_inter'].append(img)
        return img, intermediates

    def _decode(self, x_latent, cond, t_start, scale, uc, args, callback):
        if t_start > len(self.ddim_timesteps):
            raise ValueError(f'{type(self).__name__}.decode: t_start {t_start} > {len(self.ddim_timesteps)} schedule steps')
        if t_start <= 0:
            return x_latent
        return self._run(x_latent, cond, int(t_start), scale, uc, args, callback)

    # the loop over the first n table entries, newest first
    # trace = (log_every_t, the intermediates dict to append to) or None; phi: the engaged guidance rescale (0: off)
    def _run(self, img, cond, n, scale, uc, args, callback, mask=None, x0=None, trace=None, phi=0.0, seeds=None):
        s, ddim = self.solver, self._ddim
        timesteps = self.ddim_timesteps[:n]
        a = [float(v) for v in self.ddim_alphas[:n]]
        ap = [float(v) for v in self.ddim_alphas_prev[:n]]
        fast = getattr(self.model, s.loop_hook, None)
        if fast is not None and callback is None:
            # the whole loop runs inside libmkd (mkd_<loop>); masked: the blend's draws are taken here in loop order, as DDIMSampler
            # does, with the DDPM tables at each entry's timestep
            kw = {} if mask is None else blend_kwargs(ddim._q_tables(), x0, mask, timesteps, seeds)
            return fast_loop(fast, img, cond, (timesteps, a, ap, *args), scale, uc, kw, trace, phi)
        step_fn = getattr(self.model, s.step, None)
        on_device = step_fn is not None and img.is_cuda
        # on the device the floats the in-library loop uses; host tensors (plumbing with a stand-in model, e.g. CPU tests): the same
        # formulae in torch
        coef, _ = (s.device_table if on_device else s.host_table)(a, ap, *args)
        state = [None] * (s.carried + s.depth)          # the carried latents, then m_{k-1}, m_{k-2}, ...

        def step(img, ts, index, k):
            e_c, e_u = ddim._eps(img, cond, ts, scale, uc)
            carried, hist = state[:s.carried], state[s.carried:]
            if on_device:
                rescale = e_u is not None and phi != 0.0
                out = step_fn(img, *carried, e_c, e_u, scale, coef[index], *hist, **({'guidance_rescale': phi} if rescale else {}))
            else:
                out = s.host_update(img, *carried, guided_eps(e_c, e_u, scale, phi), [float(v) for v in coef[index]], *hist)
            state[:] = [*out[1:-1], out[-1], *hist[:-1]]
            return out[0], out[-1]

        blend = None if mask is None else (lambda t, img, k: ddim._q_blend(x0, t, mask, img, seeds=seeds, row=k))
        return step_loop(img, timesteps, step, callback, blend, trace)
