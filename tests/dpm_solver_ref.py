"""float64 restatement of the multistep DPM-Solver++ (test infrastructure only): Lu et al. 2022, Algorithm 2, in the form of the
published dpm_solver's multistep_dpm_solver_{second,third}_update (data prediction, solver_type 'dpmsolver'), on a DDIM step grid:
table entry i goes from a_t = alphas[i] to a_prev = alphas_prev[i], the model is evaluated at timesteps[i], the loop runs
i = n-1 .. 0.  Written over the difference quotients D1 / D2, not over per-step coefficients: ``coefficients`` recovers those by
linearity, so the library's table is checked against an independent derivation."""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from oracle import sampler

Tensor = torch.Tensor


def lam(a: float) -> float:
    """half log-SNR: log(alpha / sigma) with alpha = sqrt(a), sigma = sqrt(1 - a)"""
    return 0.5 * math.log(a / (1.0 - a))


def grid(S: int, sch: Optional['sampler.Schedule'] = None):
    """exactly S table entries on the uniform DDIM grid (make_ddim's own when S divides the schedule length):
    (timesteps int64 [S], alphas float32 [S], alphas_prev float32 [S])"""
    sch = sch or sampler.Schedule()
    ts = np.arange(S) * (sch.num_timesteps // S) + 1
    ac = sch.alphas_cumprod.numpy()
    return ts, ac[ts].astype(np.float32), np.asarray([ac[0]] + ac[ts[:-1]].tolist(), dtype=np.float32)


def step_orders(n: int, order: int, lower_order_final: bool = True) -> List[int]:
    """order of executed step k = 0 .. n-1: min(order, k + 1), and with lower_order_final and n < 10 at most n - k"""
    out = []
    for k in range(n):
        p = min(order, k + 1)
        if lower_order_final and n < 10:
            p = min(p, n - k)
        out.append(p)
    return out


def update(x, m0, m1, m2, a_t: float, a_p: float, lam_1: float, lam_2: float, p: int):
    """one multistep update of order p from the x0-predictions m0 (this step), m1, m2 (the previous two, evaluated at lambda lam_1,
    lam_2); floats or tensors"""
    lam_t = lam(a_t)
    h = lam(a_p) - lam_t
    phi_1 = math.expm1(-h)
    sig = math.sqrt(1.0 - a_p) / math.sqrt(1.0 - a_t)
    alpha_p = math.sqrt(a_p)
    if p == 1:
        return sig * x - alpha_p * phi_1 * m0
    r0 = (lam_t - lam_1) / h
    D1_0 = (1.0 / r0) * (m0 - m1)
    if p == 2:
        return sig * x - alpha_p * phi_1 * m0 - 0.5 * (alpha_p * phi_1) * D1_0
    r1 = (lam_1 - lam_2) / h
    D1_1 = (1.0 / r1) * (m1 - m2)
    D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
    D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
    phi_2 = phi_1 / h + 1.0
    phi_3 = phi_2 / h - 0.5
    return sig * x - alpha_p * phi_1 * m0 + alpha_p * phi_2 * D1 - alpha_p * phi_3 * D2


def coefficients(alphas: Sequence[float], alphas_prev: Sequence[float], order: int, lower_order_final: bool = True):
    """float64 [n, 6] = 1/alpha_t, sigma_t, c_x, c_0, c_1, c_2 per table entry (the update is linear in x, m0, m1, m2: each
    coefficient is the update of a unit input), and the step orders [n] indexed like the table"""
    n = len(alphas)
    orders = step_orders(n, order, lower_order_final)
    coef = np.zeros((n, 6))
    by_entry = np.zeros(n, dtype=np.int64)
    lams: List[float] = []
    for k in range(n):
        i = n - 1 - k
        a_t, a_p = float(alphas[i]), float(alphas_prev[i])
        l1 = lams[-1] if k >= 1 else 0.0
        l2 = lams[-2] if k >= 2 else 0.0
        unit = lambda *v: update(*v, a_t, a_p, l1, l2, orders[k])
        coef[i] = (1.0 / math.sqrt(a_t), math.sqrt(1.0 - a_t), unit(1.0, 0.0, 0.0, 0.0), unit(0.0, 1.0, 0.0, 0.0),
                   unit(0.0, 0.0, 1.0, 0.0) if orders[k] >= 2 else 0.0, unit(0.0, 0.0, 0.0, 1.0) if orders[k] >= 3 else 0.0)
        by_entry[i] = orders[k]
        lams.append(lam(a_t))
    return coef, by_entry


def dpm_solver_pp(eps_fn: Callable, timesteps, alphas, alphas_prev, x_T: Tensor, cond=None, order: int = 2,
                  lower_order_final: bool = True, scale: float = 1.0, uc=None, blend: Optional[Callable] = None,
                  trace: Optional[list] = None) -> Tensor:
    """The loop: eps_fn(x, ts, cond) like masked_sampling_ref.masked_ddim's; guidance batches [uncond; cond] through one evaluation and
    combines e = e_u + scale (e_c - e_u).  blend(k, step, img) (optional) is applied before executed step k (masked sampling).
    Runs in the dtype of x_T with float64 scalars."""
    n = len(timesteps)
    orders = step_orders(n, order, lower_order_final)
    img = x_T
    hist: List[Tensor] = []
    lams: List[float] = []
    for k in range(n):
        i = n - 1 - k
        step = int(timesteps[i])
        a_t, a_p = float(alphas[i]), float(alphas_prev[i])
        if blend is not None:
            img = blend(k, step, img)
        ts = torch.full((x_T.shape[0],), step, dtype=torch.long)
        if uc is None or scale == 1.0:
            e = eps_fn(img, ts, cond)
        else:
            cc = {key: (None if cond[key] is None else [torch.cat([u, v]) for u, v in zip(uc[key], cond[key])]) for key in cond}
            e_u, e_c = eps_fn(torch.cat([img, img]), torch.cat([ts, ts]), cc).chunk(2)
            e = e_u + scale * (e_c - e_u)
        m0 = (img - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
        m1 = hist[-1] if k >= 1 else None
        m2 = hist[-2] if k >= 2 else None
        img = update(img, m0, m1, m2, a_t, a_p, lams[-1] if k >= 1 else 0.0, lams[-2] if k >= 2 else 0.0, orders[k])
        hist.append(m0)
        lams.append(lam(a_t))
        if trace is not None:
            trace.append(img)
    return img


def step_fp64(x: Tensor, e_c: Tensor, e_u: Optional[Tensor], scale: float, coef6, m1: Optional[Tensor], m2: Optional[Tensor]):
    """one update from given fp32 coefficients in float64: (x_prev, m0, the magnitude sum |c_x x| + sum |c_j m_j|, the magnitude sum of m0)"""
    k = [float(np.float32(v)) for v in coef6]
    s = float(np.float32(scale))
    x, e_c = x.double(), e_c.double()
    if e_u is None:
        e, emag = e_c, e_c.abs()
    else:
        e_u = e_u.double()
        e, emag = e_u + s * (e_c - e_u), e_u.abs() + abs(s) * (e_c - e_u).abs()
    m0 = (x - k[1] * e) * k[0]
    m0mag = (x.abs() + k[1] * emag) * k[0]
    out = k[2] * x + k[3] * m0
    mag = (k[2] * x).abs() + (k[3] * m0).abs()
    if k[4] != 0.0:
        out = out + k[4] * m1.double(); mag = mag + (k[4] * m1.double()).abs()
    if k[5] != 0.0:
        out = out + k[5] * m2.double(); mag = mag + (k[5] * m2.double()).abs()
    return out, m0, mag, m0mag
