"""UniPC predictor-corrector sampler (host logic): the unified predictor-corrector framework of Zhao et al. 2023 in its data-prediction
"bh2" form, deterministic, eps parameterisation, on the step grid and tables of ``DDIMSampler.make_schedule(S)`` exactly as
``dpm_solver.py`` uses them.  The definition is include/mkd.h's (mkd_unipc_table): a multistep predictor plus a corrector that re-uses
the evaluation the next step needs anyway, so a loop of n steps costs n evaluations.  Every step is two linear forms over the predicted
latent x~_k the model is evaluated at, the corrected latent x^c carried beside it and the last four x0-predictions m_k = (x~_k - sigma_k e_k) / alpha_k:

    x^c_k    = a_c x^c_{k-1} + q_0 m_k + q_1 m_{k-1} + q_2 m_{k-2} + q_3 m_{k-3}        (a_c == 0: no corrector, x^c_k = x~_k)
    x~_{k+1} = a_p x^c_k + p_0 m_k + p_1 m_{k-1} + p_2 m_{k-2}

with twelve schedule-only numbers per step.  Order 2 with the corrector off is the DPM-Solver++ 2M trajectory; order 1 with the corrector
off is algebraically the eta = 0 DDIM loop.  What is shown for it is arithmetic, polynomial exactness and a Gaussian toy;
image quality at low evaluation counts is not shown: there are no pretrained weights here.
This module holds the coefficients; the class is ``sampling.MultistepSampler`` with the 'unipc' record (the host update is there too)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .sampling import SOLVERS, MultistepSampler

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


class UniPCSampler(MultistepSampler):
    solver = SOLVERS['unipc']

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
               order=2, lower_order_final=True, corrector=True, callback=None, mask=None, x0=None, log_every_t=100, guidance_rescale=0.0,
               seeds=None, **kw):
        """intermediates as DDIMSampler's: x_inter / pred_x0 = [x_T, one entry per step with index % log_every_t == 0 or the first
        executed one] (x_inter: the predicted latent x~_{k+1} after the step; pred_x0: the solver's m_k), from the in-library loop's
        trace or the step loop alike.  guidance_rescale = phi in [0, 1], engaged with guidance and phi > 0.  ``seeds``
        (as DDIMSampler.sample's): x_T from noise.normal on stream 0 unless given -- this solver's only draw; no torch generator is advanced.
        mask / x0 are refused: masked sampling is not defined for this solver."""
        return self._sample(S, batch_size, shape, conditioning, x_T, unconditional_guidance_scale, unconditional_conditioning,
                            (order, lower_order_final, bool(corrector)), callback, mask, x0, log_every_t, guidance_rescale, seeds, kw)

    def sample_specs(self, *args, **kwargs):
        raise NotImplementedError('UniPCSampler: per-sample specs are not built for this solver (mkd_sample_rows runs DDIM and '
                                  'DPM-Solver++ only)')

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None, order=2,
               lower_order_final=True, corrector=True, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first, on the schedule of the last make_schedule: regenerates a latent
        inverted with DDIMSampler.encode(x0, t_enc=t_start).  t_start is one number for the batch."""
        return self._decode(x_latent, cond, t_start, unconditional_guidance_scale, unconditional_conditioning,
                            (order, lower_order_final, bool(corrector)), callback)
