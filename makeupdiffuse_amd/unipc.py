"""UniPC predictor-corrector sampler (host logic): the unified predictor-corrector framework of Zhao et al. 2023 in its data-prediction
"bh2" form, deterministic, eps parameterisation, on the step grid and tables of ``DDIMSampler.make_schedule(S)`` exactly as
``dpm_solver.py`` uses them.  The definition is include/mkd.h's (mkd_unipc_table): a multistep predictor plus a corrector that re-uses
the evaluation the next step needs anyway, so a loop of n steps costs n evaluations.  Every step is two linear forms over the predicted
latent x~_k the model is evaluated at, the corrected latent x^c carried beside it and the last four x0-predictions m_k = (x~_k - sigma_k e_k) / alpha_k:

    x^c_k    = a_c x^c_{k-1} + q_0 m_k + q_1 m_{k-1} + q_2 m_{k-2} + q_3 m_{k-3}        (a_c == 0: no corrector, x^c_k = x~_k)
    x~_{k+1} = a_p x^c_k + p_0 m_k + p_1 m_{k-1} + p_2 m_{k-2}

with twelve schedule-only numbers per step.  Order 2 with the corrector off is the DPM-Solver++ 2M trajectory; order 1 with the corrector
off is algebraically the eta = 0 DDIM loop.  What is shown for it is arithmetic, polynomial exactness and a Gaussian toy;
image quality at low evaluation counts is not shown: there are no pretrained weights here."""
from __future__ import annotations

import math

import numpy as np
import torch

from .ddim import DDIMSampler, _check_rescale, _check_seeds, rescale_guided_eps

__all__ = ['UniPCSampler', 'unipc_coefficients']


def _psi(h):
    """psi_0 .. psi_3 of h > 0: psi_0 = 1 - e^-h, psi_j = h^j / j! - psi_{j-1}; below h = 1 by the alternating series
    sum_m (-1)^m h^(j+1+m) / (j+1+m)! (the recursion cancels there)"""
    if h < 1.0:
        out = []
        for j in range(4):
            term = 1.0
            for i in range(1, j + 2):
                term *= h / i
            s = 0.0
            for m in range(40):
                if term == 0.0:
                    break
                s += term
                term *= -h / (j + 2 + m)
            out.append(s)
        return out
    out = [-math.expm1(-h)]
    pw = 1.0
    for j in range(1, 4):
        pw *= h / j
        out.append(pw - out[-1])
    return out


def _weights(r, h, psi):
    """w of one update over the nodes r: sum_j w_j r_j^i = i! psi_i / h^i for i = 1 .. q (Gaussian elimination with partial pivoting);
    q == 1: the shortcut psi_0 / (2 r)"""
    q = len(r)
    if q == 0:
        return []
    if q == 1:
        if r[0] == 0.0:
            raise ValueError('UniPC: the grid does not determine the weights')
        return [psi[0] / (2.0 * r[0])]
    A = [[0.0] * (q + 1) for _ in range(q)]
    fact = hp = 1.0
    for i in range(1, q + 1):
        fact *= i
        hp *= h
        for j in range(q):
            A[i - 1][j] = math.pow(r[j], i)
        A[i - 1][q] = fact * psi[i] / hp
    for c in range(q):
        piv = c
        for i in range(c + 1, q):
            if abs(A[i][c]) > abs(A[piv][c]):
                piv = i
        if not abs(A[piv][c]) > 0.0:
            raise ValueError('UniPC: the grid does not determine the weights')
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
        for i in range(c + 1, q):
            f = A[i][c] / A[c][c]
            for j in range(c, q + 1):
                A[i][j] -= f * A[c][j]
    w = [0.0] * q
    for c in range(q - 1, -1, -1):
        s = A[c][q]
        for j in range(c + 1, q):
            s -= A[c][j] * w[j]
        w[c] = s / A[c][c]
    return w


def unipc_coefficients(alphas, alphas_prev, order=2, lower_order_final=True, corrector=True):
    """float64 ``(coef [n, 12], step_order [n])`` of UniPC on a DDIM table: row i = 1/alpha, sigma, a_c, q_0 .. q_3, a_p, p_0 .. p_2, 0 of
    table entry i (executed step k = n - 1 - i).  The same arithmetic as mkd_unipc_table, which stores it as float."""
    n = len(alphas)
    if order not in (1, 2, 3):
        raise ValueError('UniPC: order must be 1, 2 or 3')
    if n <= 0 or len(alphas_prev) != n:
        raise ValueError('UniPC: alphas / alphas_prev must be non-empty and equally long')
    al, ap = [float(v) for v in alphas], [float(v) for v in alphas_prev]
    if not all(0.0 < v < 1.0 for v in al + ap):
        raise ValueError('UniPC: every alpha must lie in (0, 1)')
    if any(ap[i] != al[i - 1] for i in range(1, n)):
        raise ValueError('UniPC: the table must be contiguous (alphas_prev[i] == alphas[i - 1]): the corrector walks from one '
                         'evaluation point to the next')
    a = [al[n - 1 - k] for k in range(n)] + [ap[0]]          # grid point k = 0 .. n
    lam = [0.5 * math.log(v / (1.0 - v)) for v in a]
    if any(not lam[k] > lam[k - 1] for k in range(1, n + 1)):
        raise ValueError('UniPC: lambda must increase along the executed steps')
    p = [min(order, k + 1) for k in range(n)]
    if lower_order_final and n < 10:
        p = [min(p[k], n - k) for k in range(n)]
    coef = np.zeros((n, 12), dtype=np.float64)
    orders = np.zeros(n, dtype=np.int32)
    for k in range(n):
        o = coef[n - 1 - k]
        o[0], o[1] = 1.0 / math.sqrt(a[k]), math.sqrt(1.0 - a[k])
        if corrector and k >= 1:          # from base k - 1 to lambda_k: the p_{k-1} - 1 evaluations before the base, then m_k at r = 1
            q = p[k - 1]
            h = lam[k] - lam[k - 1]
            psi = _psi(h)
            w = _weights([(lam[k - 1 - j] - lam[k - 1]) / h for j in range(1, q)] + [1.0], h, psi)
            alpha = math.sqrt(a[k])
            o[2] = math.sqrt(1.0 - a[k]) / math.sqrt(1.0 - a[k - 1])
            o[3] = alpha * w[q - 1]
            o[4] = alpha * (psi[0] - sum(w))
            for j in range(1, q):
                o[4 + j] = alpha * w[j - 1]
        q = p[k] - 1                      # from base k to lambda_{k+1}: the p_k - 1 evaluations before the base
        h = lam[k + 1] - lam[k]
        psi = _psi(h)
        w = _weights([(lam[k - j] - lam[k]) / h for j in range(1, q + 1)], h, psi)
        alpha = math.sqrt(a[k + 1])
        o[7] = math.sqrt(1.0 - a[k + 1]) / math.sqrt(1.0 - a[k])
        o[8] = alpha * (psi[0] - sum(w))
        for j in range(1, q + 1):
            o[8 + j] = alpha * w[j - 1]
        orders[n - 1 - k] = p[k]
    return coef, orders


class UniPCSampler:
    # options of upstream samplers that this deterministic solver does not have
    _REJECTED = ('score_corrector', 'corrector_kwargs', 'dynamic_threshold', 'ucg_schedule', 'img_callback', 'quantize_x0')

    def __init__(self, model, **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self._ddim = DDIMSampler(model)          # the step grid, its tables and the guidance batching

    def make_schedule(self, num_steps, verbose=False):
        """The grid of DDIMSampler.make_schedule(num_steps): ddim_timesteps / ddim_alphas / ddim_alphas_prev."""
        self._ddim.make_schedule(ddim_num_steps=num_steps, ddim_eta=0.0, verbose=verbose)
        self.ddim_timesteps = self._ddim.ddim_timesteps
        self.ddim_alphas = self._ddim.ddim_alphas
        self.ddim_alphas_prev = self._ddim.ddim_alphas_prev

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
               order=2, lower_order_final=True, corrector=True, callback=None, mask=None, x0=None, log_every_t=100, guidance_rescale=0.0,
               seeds=None, **kw):
        """intermediates as DDIMSampler's: x_inter / pred_x0 = [x_T, one entry per step with index % log_every_t == 0 or the first
        executed one] (x_inter: the predicted latent x~_{k+1} after the step; pred_x0: the solver's m_k), from the in-library loop's
        trace or the step loop alike.  guidance_rescale = phi in [0, 1], engaged with guidance and phi > 0.  ``seeds``
        (as DDIMSampler.sample's): x_T from noise.normal on stream 0 unless given -- this solver's only draw; no torch generator is advanced."""
        if kw.get('eta') not in (None, 0, 0.0):
            raise NotImplementedError('UniPCSampler is deterministic: eta is not an option of UniPC')
        for k in self._REJECTED:
            if kw.get(k) not in (None, False):
                raise NotImplementedError(f'UniPCSampler.sample option {k} is not on the MakeupDiffuse path')
        if kw.get('temperature', 1.0) != 1.0 or kw.get('noise_dropout', 0.0) != 0.0:
            raise NotImplementedError('UniPCSampler draws no noise: temperature / noise_dropout do not apply')
        if mask is not None or x0 is not None:
            raise NotImplementedError('UniPCSampler: masked sampling (mask / x0) is not defined for this solver: the blend would have '
                                      'to act on the two latents it carries')
        if order not in (1, 2, 3):
            raise ValueError('UniPCSampler: order must be 1, 2 or 3')
        C, H, W = shape
        size = (batch_size, C, H, W)
        phi = _check_rescale(guidance_rescale)
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.0:
            phi = 0.0          # no unconditional half: not engaged
        if int(log_every_t) < 1:
            raise ValueError(f'log_every_t must be >= 1, got {log_every_t}')
        if seeds is not None:
            seeds = _check_seeds(seeds, batch_size)
        self.make_schedule(S, verbose=False)
        if x_T is None and seeds is not None:
            from .noise import STREAM_START, normal
            img = normal(seeds, size[1:], stream=STREAM_START, device=self.model.device)
        else:
            img = torch.randn(size, device=self.model.device) if x_T is None else x_T
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        img = self._loop(img, conditioning, len(self.ddim_timesteps), unconditional_guidance_scale, unconditional_conditioning, order,
                         lower_order_final, corrector, callback, trace=(int(log_every_t), intermediates), phi=phi)
        if len(intermediates['x_inter']) == 1:          # (a hook that keeps no trace)
            intermediates['x_inter'].append(img)
        return img, intermediates

    def sample_specs(self, *args, **kwargs):
        raise NotImplementedError('UniPCSampler: per-sample specs are not built for this solver (mkd_sample_rows runs DDIM and '
                                  'DPM-Solver++ only)')

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None, order=2,
               lower_order_final=True, corrector=True, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first, on the schedule of the last make_schedule: regenerates a latent
        inverted with DDIMSampler.encode(x0, t_enc=t_start).  t_start is one number for the batch."""
        if t_start > len(self.ddim_timesteps):
            raise ValueError(f'UniPCSampler.decode: t_start {t_start} > {len(self.ddim_timesteps)} schedule steps')
        if t_start <= 0:
            return x_latent
        return self._loop(x_latent, cond, int(t_start), unconditional_guidance_scale, unconditional_conditioning, order, lower_order_final,
                          corrector, callback)

    # the loop over the first n table entries, newest first
    # trace = (log_every_t, the intermediates dict to append to) or None; phi: the engaged guidance rescale (0: off)
    def _loop(self, img, cond, n, scale, uc, order, lower_order_final, corrector, callback, trace=None, phi=0.0):
        timesteps = self.ddim_timesteps[:n]
        a = [float(v) for v in self.ddim_alphas[:n]]
        ap = [float(v) for v in self.ddim_alphas_prev[:n]]
        fast = getattr(self.model, 'sample_loop_unipc', None)
        if fast is not None and callback is None:          # the whole loop runs inside libmkd (mkd_sample_unipc)
            kw = {}
            if trace is not None:
                kw['log_every_t'] = trace[0]
            if phi != 0.0:
                kw['guidance_rescale'] = phi
            res = fast(img, cond, timesteps, a, ap, order, lower_order_final, bool(corrector), scale, uc, **kw)
            if not isinstance(res, tuple):
                return res
            img, x_rows, x0_rows = res          # (latent, x_inter rows, pred_x0 rows); the latent stays the last x_inter entry
            trace[1]['x_inter'] += [*x_rows[:-1], img]
            trace[1]['pred_x0'] += list(x0_rows)
            return img
        step_fn = getattr(self.model, 'unipc_step', None)
        on_device = step_fn is not None and img.is_cuda
        if on_device:
            from .engine import unipc_table
            coef, _ = unipc_table(a, ap, order, lower_order_final, corrector)          # the floats the in-library loop uses
        else:
            coef, _ = unipc_coefficients(a, ap, order, lower_order_final, corrector)
        hist = [None, None, None]                            # m_{k-1}, m_{k-2}, m_{k-3}
        xc = None                                            # x^c_{k-1}
        for k in range(n):
            index = n - 1 - k
            step = int(timesteps[index])
            ts = torch.full((img.shape[0],), step, device=img.device, dtype=torch.long)
            e_c, e_u = self._ddim._eps(img, cond, ts, scale, uc)
            rescale = e_u is not None and phi != 0.0
            if on_device:
                img, xc, m0 = step_fn(img, xc, e_c, e_u, scale, coef[index], hist[0], hist[1], hist[2],
                                      **({'guidance_rescale': phi} if rescale else {}))
            else:
                # host tensors (plumbing with a stand-in model, e.g. CPU tests): the same formulae in torch
                c = [float(v) for v in coef[index]]
                if rescale:
                    e_t = rescale_guided_eps(e_c, e_u, scale, phi)
                else:
                    e_t = e_c if e_u is None else e_u + scale * (e_c - e_u)
                m0 = (img - c[1] * e_t) * c[0]
                if c[2] != 0.0:
                    xc = c[2] * xc + c[3] * m0
                    for cj, mj in zip(c[4:7], hist):
                        if cj != 0.0:
                            xc = xc + cj * mj
                else:
                    xc = img
                img = c[7] * xc + c[8] * m0
                for cj, mj in zip(c[9:11], hist):
                    if cj != 0.0:
                        img = img + cj * mj
            hist = [m0, hist[0], hist[1]]
            if callback:
                callback(k)
            if trace is not None and (index % trace[0] == 0 or index == n - 1):
                trace[1]['x_inter'].append(img)
                trace[1]['pred_x0'].append(m0)
        return img
