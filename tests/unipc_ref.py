"""float64 restatement of the UniPC predictor-corrector (test infrastructure only), written from the definition in include/mkd.h, not
from the library's table: one ``update`` over nodes with the weights solved by numpy.linalg.solve, the loop over it, the per-step rows
recovered by linearity (``coefficients``), the float64 form of one kernel step with its magnitude sums (``step_fp64``) and the Gaussian
toy with its exact ODE solution.  Grid point k = 0 .. n-1 is the evaluation of executed step k (table entry n-1-k), grid point n is
alphas_prev[0]."""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from dpm_solver_ref import grid, lam, step_orders          # noqa: F401  (the same grid and order rule)

Tensor = torch.Tensor


def psi(j: int, h: float) -> float:
    """psi_j(h) = int_0^h e^(u-h) u^j / j! du = sum_{m >= 0} (-1)^m h^(j+1+m) / (j+1+m)!  (psi_0 = 1 - e^-h, psi_j = h^j / j! - psi_{j-1}),
    summed exactly-rounded; the alternating terms stay below e^h, so for the h of these grids (< 4) the cancellation costs ~1e-15"""
    terms, t = [], 1.0
    for i in range(1, j + 2):
        t *= h / i
    for m in range(80):
        terms.append(t)
        t *= -h / (j + 2 + m)
    return math.fsum(terms)


def grid_points(alphas: Sequence[float], alphas_prev: Sequence[float]) -> List[float]:
    """alphas_cumprod at grid points 0 .. n of a contiguous table (ValueError otherwise)"""
    n = len(alphas)
    if any(float(alphas_prev[i]) != float(alphas[i - 1]) for i in range(1, n)):
        raise ValueError('the table is not contiguous')
    return [float(alphas[n - 1 - k]) for k in range(n)] + [float(alphas_prev[0])]


def weights(r: Sequence[float], h: float, kind: str, shortcut: bool = True) -> np.ndarray:
    """w of one update: sum_j w_j r_j^i = i! psi_i(h) / h^i for i = 1 .. q.  With one node the published "bh2" shortcuts apply
    (shortcut False: the solved weight): predictor psi_0 / (2 r_1), corrector psi_0 / 2"""
    q = len(r)
    if q == 0:
        return np.zeros(0)
    if q == 1 and shortcut:
        return np.array([psi(0, h) / (2.0 * r[0]) if kind == 'predictor' else psi(0, h) / 2.0])
    A = np.array([[rj ** i for rj in r] for i in range(1, q + 1)], dtype=np.float64)
    b = np.array([math.factorial(i) * psi(i, h) / h ** i for i in range(1, q + 1)], dtype=np.float64)
    return np.linalg.solve(A, b)


def update(x_s, m_s, a_s: float, a_t: float, nodes, kind: str, shortcut: bool = True):
    """U from the base (x_s, m_s) at alphas_cumprod a_s to a_t over ``nodes`` = [(lambda_node, m_node), ...]; floats, arrays or tensors"""
    h = lam(a_t) - lam(a_s)
    r = [(ln - lam(a_s)) / h for ln, _ in nodes]
    w = weights(r, h, kind, shortcut)
    acc = psi(0, h) * m_s
    for wj, (_, mj) in zip(w, nodes):
        acc = acc + float(wj) * (mj - m_s)
    return (math.sqrt(1.0 - a_t) / math.sqrt(1.0 - a_s)) * x_s + math.sqrt(a_t) * acc


def run(m_fn: Callable, alphas, alphas_prev, x_T, order: int = 2, lower_order_final: bool = True, corrector: bool = True,
        trace: Optional[list] = None):
    """The loop of the definition.  m_fn(k, x) -> the x0-prediction m_k at the predicted latent x = x~_k of executed step k.  trace: gets
    (x~_{k+1}, x^c_k, m_k) per step"""
    a = grid_points(alphas, alphas_prev)
    n = len(alphas)
    p = step_orders(n, order, lower_order_final)
    lams = [lam(v) for v in a]
    x, xc, ms = x_T, None, []
    for k in range(n):
        m_k = m_fn(k, x)
        if k >= 1 and corrector:
            nodes = [(lams[k - 1 - j], ms[k - 1 - j]) for j in range(1, p[k - 1])] + [(lams[k], m_k)]
            xc = update(xc, ms[k - 1], a[k - 1], a[k], nodes, 'corrector')
        else:
            xc = x
        nodes = [(lams[k - j], ms[k - j]) for j in range(1, p[k])]
        x = update(xc, m_k, a[k], a[k + 1], nodes, 'predictor')
        ms.append(m_k)
        if trace is not None:
            trace.append((x, xc, m_k))
    return x


def coefficients(alphas, alphas_prev, order: int, lower_order_final: bool = True, corrector: bool = True):
    """float64 [n, 12] = 1/alpha, sigma, a_c, q_0 .. q_3, a_p, p_0 .. p_2, 0 per table entry (both forms are linear in their inputs: each
    coefficient is the update of a unit input), and the step orders [n] indexed like the table"""
    a = grid_points(alphas, alphas_prev)
    n = len(alphas)
    p = step_orders(n, order, lower_order_final)
    lams = [lam(v) for v in a]
    coef = np.zeros((n, 12))
    for k in range(n):
        o = coef[n - 1 - k]
        o[0], o[1] = 1.0 / math.sqrt(a[k]), math.sqrt(1.0 - a[k])
        if k >= 1 and corrector:
            q = p[k - 1]
            # inputs: xc_prev, m_k, m_{k-1} (the base), m_{k-2}, m_{k-3}
            def cor(xc, m0, m1, m2, m3):
                hist = [m2, m3]
                return update(xc, m1, a[k - 1], a[k], [(lams[k - 1 - j], hist[j - 1]) for j in range(1, q)] + [(lams[k], m0)], 'corrector')
            for j in range(5):
                unit = [0.0] * 5
                unit[j] = 1.0
                if j <= 2 or j - 2 < q:
                    o[2 + j] = cor(*unit)
        q = p[k] - 1
        # inputs: xc, m_k (the base), m_{k-1}, m_{k-2}
        def pre(xc, m0, m1, m2):
            hist = [m1, m2]
            return update(xc, m0, a[k], a[k + 1], [(lams[k - j], hist[j - 1]) for j in range(1, q + 1)], 'predictor')
        for j in range(4):
            unit = [0.0] * 4
            unit[j] = 1.0
            if j <= 1 or j - 1 <= q:
                o[7 + j] = pre(*unit)
    by_entry = np.asarray(p[::-1], dtype=np.int64)
    return coef, by_entry


def run_rows(m_fn: Callable, coef, x_T, trace: Optional[list] = None):
    """the two linear forms driven from a [n, 12] table (an all-zero corrector, a_c == 0, means x^c_k = x~_k)"""
    n = len(coef)
    x, xc, hist = x_T, None, [None, None, None]
    for k in range(n):
        c = [float(v) for v in coef[n - 1 - k]]
        m0 = m_fn(k, x)
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
        hist = [m0, hist[0], hist[1]]
        if trace is not None:
            trace.append((x, xc, m0))
    return x


def unipc(eps_fn: Callable, timesteps, alphas, alphas_prev, x_T: Tensor, cond=None, order: int = 2, lower_order_final: bool = True,
          corrector: bool = True, scale: float = 1.0, uc=None, trace: Optional[list] = None) -> Tensor:
    """The loop around a model: eps_fn(x, ts, cond) like dpm_solver_ref.dpm_solver_pp's; guidance batches [uncond; cond] through one
    evaluation and combines e = e_u + scale (e_c - e_u).  Runs in the dtype of x_T with float64 scalars."""
    n = len(timesteps)

    def m_fn(k, img):
        i = n - 1 - k
        a_t = float(alphas[i])
        ts = torch.full((x_T.shape[0],), int(timesteps[i]), dtype=torch.long)
        if uc is None or scale == 1.0:
            e = eps_fn(img, ts, cond)
        else:
            cc = {key: (None if cond[key] is None else [torch.cat([u, v]) for u, v in zip(uc[key], cond[key])]) for key in cond}
            e_u, e_c = eps_fn(torch.cat([img, img]), torch.cat([ts, ts]), cc).chunk(2)
            e = e_u + scale * (e_c - e_u)
        return (img - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
    return run(m_fn, alphas, alphas_prev, x_T, order, lower_order_final, corrector, trace)


def step_fp64(x: Tensor, xc_prev: Tensor, e_c: Tensor, e_u: Optional[Tensor], scale: float, coef12, m1: Tensor, m2: Tensor, m3: Tensor,
              e_mag: Optional[Tensor] = None):
    """one kernel step from given fp32 coefficients in float64: (x_next, xc, m0) and their magnitude sums, the sums of the absolute
    values of the terms each output is made of, with the magnitude sum of an fp32 intermediate standing in for it in the outputs built
    on it (m0 in xc and x_next, xc in x_next).  e_mag (with e_u None): the magnitude sum of an eps that e_c holds already combined"""
    c = [float(np.float32(v)) for v in coef12]
    s = float(np.float32(scale))
    x, e_c = x.double(), e_c.double()
    if e_u is None:
        e, emag = e_c, (e_c.abs() if e_mag is None else e_mag.double())
    else:
        e_u = e_u.double()
        e, emag = e_u + s * (e_c - e_u), e_u.abs() + abs(s) * (e_c - e_u).abs()
    m0 = (x - c[1] * e) * c[0]
    m0mag = (x.abs() + c[1] * emag) * c[0]
    hist = [m1.double(), m2.double(), m3.double()]
    if c[2] != 0.0:
        xc = c[2] * xc_prev.double() + c[3] * m0
        xcmag = (c[2] * xc_prev.double()).abs() + abs(c[3]) * m0mag
        for cj, mj in zip(c[4:7], hist):
            if cj != 0.0:
                xc = xc + cj * mj
                xcmag = xcmag + (cj * mj).abs()
    else:
        xc, xcmag = x, x.abs()
    out = c[7] * xc + c[8] * m0
    mag = abs(c[7]) * xcmag + abs(c[8]) * m0mag
    for cj, mj in zip(c[9:11], hist):
        if cj != 0.0:
            out = out + cj * mj
            mag = mag + (cj * mj).abs()
    return (out, xc, m0), (mag, xcmag, m0mag)


# ---- the Gaussian toy: data N(mu, diag(v)) in D dimensions; eps and the probability-flow ODE are analytic ------------------------------
class GaussianToy:
    def __init__(self, dim: int = 64, seed: int = 0):
        rng = np.random.default_rng(seed)
        self.mu = rng.standard_normal(dim)
        self.v = np.exp(rng.uniform(math.log(0.05), math.log(4.0), dim))          # per-dimension data variance
        self.z = rng.standard_normal(dim)

    def var(self, a: float):
        return a * self.v + (1.0 - a)

    def x_at(self, a: float):
        """the ODE solution through the start point, at alphas_cumprod a: x = alpha mu + sqrt(var(a)) z"""
        return math.sqrt(a) * self.mu + np.sqrt(self.var(a)) * self.z

    def m(self, a: float, x):
        """x0-prediction of the exact eps = sigma (x - alpha mu) / var(a) at alphas_cumprod a"""
        al, sg = math.sqrt(a), math.sqrt(1.0 - a)
        e = sg * (x - al * self.mu) / self.var(a)
        return (x - sg * e) / al

    def errors(self, S: int, solve: Callable):
        """rel. error of the final latent of solve(m_fn, alphas, alphas_prev, x_T) on the S-entry uniform grid"""
        _, al, ap = grid(S)
        a = grid_points(al, ap)
        out = solve(lambda k, x: self.m(a[k], x), al, ap, self.x_at(a[0]))
        exact = self.x_at(a[-1])
        return float(np.linalg.norm(out - exact) / np.linalg.norm(exact))
