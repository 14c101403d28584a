"""Restatement of the per-sample loop (one request row per sample in one batch) for the tests.

  * the two per-sample updates in float64 from step-table entries (with the magnitude sums the kernel bounds are stated in), and
  * the whole loop over the oracle's single-request pieces: ``oracle.sampler.denoising_step`` per sample for DDIM,
    ``dpm_solver_ref.update`` per sample for DPM-Solver++, around ONE evaluation of the batch per executed step in which every
    sample has its own timestep.

Executed step k = 0 .. S_max - 1: sample b is active while k < n_b and applies its table entry n_b - 1 - k; a finished sample is still
evaluated (at the timestep of its entry 0) and the result is thrown away: its row is not touched again."""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

import dpm_solver_ref as dref
from oracle import sampler

Tensor = torch.Tensor


# ---- the updates from step-table entries, float64 ------------------------------------------------------------------------------
def _guided64(e_c: Tensor, e_u: Optional[Tensor], s: float):
    e_c = e_c.double()
    if e_u is None:
        return e_c, e_c.abs()
    e_u = e_u.double()
    return e_u + s * (e_c - e_u), e_u.abs() + abs(s) * (e_c - e_u).abs()


def ddim_rows_fp64(x: Tensor, e_c: Tensor, e_u: Optional[Tensor], entries, noise: Optional[Tensor] = None, temperature: float = 1.0):
    """[B, n] tensors, entries [B] of the step table -> (x_prev, pred_x0, magnitude sum of x_prev, of pred_x0, active [B]) in float64.
    Rows of finished samples come back as NaN (nothing may be compared against them).  e = e_u + s (e_c - e_u) (e_u None: e_c),
    p0 = (x - c3 e) c0, x_prev = c1 p0 + c2 e (+ sigma noise T where sigma != 0) with c = the entry's four fp32 coefficients."""
    B = x.shape[0]
    xp = torch.full(x.shape, float('nan'), dtype=torch.float64); p0 = xp.clone(); mag = xp.clone(); mag0 = xp.clone()
    active = []
    for b in range(B):
        en = entries[b]
        active.append(bool(en['active']))
        if not en['active']:
            continue
        c = [float(v) for v in en['coef']]
        e, emag = _guided64(e_c[b], None if e_u is None else e_u[b], float(en['scale']))
        xb = x[b].double()
        p = (xb - c[3] * e) * c[0]
        pm = (xb.abs() + c[3] * emag) * c[0]
        r = c[1] * p + c[2] * e
        rm = c[1] * pm + c[2] * emag
        sg = float(en['sigma'])
        if noise is not None and sg != 0.0:
            nz = sg * noise[b].double() * float(np.float32(temperature))
            r = r + nz; rm = rm + nz.abs()
        xp[b], p0[b], mag[b], mag0[b] = r, p, rm, pm
    return xp, p0, mag, mag0, active


def dpm_rows_fp64(x: Tensor, e_c: Tensor, e_u: Optional[Tensor], entries, m1: Tensor, m2: Tensor):
    """... and the DPM-Solver++ update: (x_prev, m0, magnitude sum of x_prev, of m0, active); dpm = 1/alpha, sigma, c_x, c_0, c_1, c_2"""
    B = x.shape[0]
    xp = torch.full(x.shape, float('nan'), dtype=torch.float64); m0 = xp.clone(); mag = xp.clone(); mag0 = xp.clone()
    active = []
    for b in range(B):
        en = entries[b]
        active.append(bool(en['active']))
        if not en['active']:
            continue
        k = [float(v) for v in en['dpm']]
        e, emag = _guided64(e_c[b], None if e_u is None else e_u[b], float(en['scale']))
        xb = x[b].double()
        m = (xb - k[1] * e) * k[0]
        mm = (xb.abs() + k[1] * emag) * k[0]
        r = k[2] * xb + k[3] * m
        rm = (k[2] * xb).abs() + (k[3] * m).abs()
        if k[4] != 0.0:
            r = r + k[4] * m1[b].double(); rm = rm + (k[4] * m1[b].double()).abs()
        if k[5] != 0.0:
            r = r + k[5] * m2[b].double(); rm = rm + (k[5] * m2[b].double()).abs()
        xp[b], m0[b], mag[b], mag0[b] = r, m, rm, mm
    return xp, m0, mag, mag0, active


# ---- the whole loop over the oracle's single-request pieces ----------------------------------------------------------------------
def _eval(eps_fn: Callable, img: Tensor, ts: Tensor, cond, uc, scales: Sequence[float]) -> Tensor:
    """one evaluation of the batch, every sample at its own timestep; guided (some scale != 1): [uncond; cond] through one
    evaluation, every sample combined with its own scale (a scale of 1 inside a guided batch goes through the same expression)"""
    if all(float(s) == 1.0 for s in scales):
        return eps_fn(img, ts, cond)
    cc = sampler.cat_cond(uc, cond)
    e_u, e_c = eps_fn(torch.cat([img, img]), torch.cat([ts, ts]), cc).chunk(2)
    s = torch.tensor([float(v) for v in scales], dtype=img.dtype).view(-1, 1, 1, 1)
    return e_u + s * (e_c - e_u)


def ddim_loop_rows(eps_fn: Callable, schedules: Sequence['sampler.Schedule'], n_steps: Sequence[int], x_T: Tensor, cond,
                   scales: Optional[Sequence[float]] = None, uc=None, noise: Optional[Tensor] = None, temperature: float = 1.0) -> Tensor:
    """schedules[b] (make_ddim done by the caller) and n_steps[b] <= its entries: sample b runs entries n_b - 1 .. 0 of ITS schedule.
    noise [S_max, B, ...] or None: row k is executed step k's draw; a sample takes its slice where its sigma is non-zero."""
    B = x_T.shape[0]
    scales = [1.0] * B if scales is None else list(scales)
    img = x_T.clone()
    for k in range(max(n_steps)):
        idx = [n_steps[b] - 1 - k if k < n_steps[b] else 0 for b in range(B)]
        ts = torch.tensor([int(schedules[b].ddim_timesteps[idx[b]]) for b in range(B)], dtype=torch.long)
        e = _eval(eps_fn, img, ts, cond, uc, scales)
        nxt = img.clone()
        for b in range(B):
            if k >= n_steps[b]:
                continue          # finished: the evaluation's result for this row is discarded
            nz = None
            if noise is not None and float(schedules[b].ddim_sigmas[idx[b]]) != 0.0:
                nz = noise[k, b:b + 1]
            nxt[b:b + 1], _ = sampler.denoising_step(lambda *_: e[b:b + 1], schedules[b], img[b:b + 1], None, ts[b:b + 1], idx[b],
                                                     temperature=temperature, noise=nz)
        img = nxt
    return img


def dpm_loop_rows(eps_fn: Callable, grids, orders: Sequence[int], x_T: Tensor, cond, scales: Optional[Sequence[float]] = None,
                  uc=None, lower_order_final: bool = True) -> Tensor:
    """grids[b] = (timesteps, alphas, alphas_prev) of sample b (every entry is run), orders[b] its solver order"""
    B = x_T.shape[0]
    scales = [1.0] * B if scales is None else list(scales)
    n = [len(g[0]) for g in grids]
    step_orders = [dref.step_orders(n[b], orders[b], lower_order_final) for b in range(B)]
    hist: List[List[Tensor]] = [[] for _ in range(B)]
    lams: List[List[float]] = [[] for _ in range(B)]
    img = x_T.clone()
    for k in range(max(n)):
        idx = [n[b] - 1 - k if k < n[b] else 0 for b in range(B)]
        ts = torch.tensor([int(grids[b][0][idx[b]]) for b in range(B)], dtype=torch.long)
        e = _eval(eps_fn, img, ts, cond, uc, scales)
        nxt = img.clone()
        for b in range(B):
            if k >= n[b]:
                continue
            a_t, a_p = float(grids[b][1][idx[b]]), float(grids[b][2][idx[b]])
            xb = img[b:b + 1]
            m0 = (xb - math.sqrt(1.0 - a_t) * e[b:b + 1]) / math.sqrt(a_t)
            nxt[b:b + 1] = dref.update(xb, m0, hist[b][-1] if k >= 1 else None, hist[b][-2] if k >= 2 else None, a_t, a_p,
                                       lams[b][-1] if k >= 1 else 0.0, lams[b][-2] if k >= 2 else 0.0, step_orders[b][k])
            hist[b].append(m0)
            lams[b].append(dref.lam(a_t))
        img = nxt
    return img
