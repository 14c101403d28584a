"""Per-sample requests in one batch (host logic): a ``SampleSpec`` per sample, the tables of each built as the samplers build theirs,
the host draw order of eta > 0, and the restatement of the step table that libmkd fills (include/mkd.h mkd_step_table).

A batch served by ``MkdEngine.sample_rows`` runs ``S_max = max(steps)`` executed steps; sample b is active while k < n_b and applies its
table entry n_b - 1 - k, so all samples start together and short ones finish first."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .schedule import make_ddim_sampling_parameters, make_ddim_timesteps

MAX_STEPS = 1024          # MKD_MAX_STEPS of include/mkd.h
SOLVERS = ('ddim', 'dpmpp')


@dataclass(frozen=True)
class SampleSpec:
    """One sample's request: ``steps`` = the S of ``DDIMSampler.make_schedule`` (the uniform DDIM grid; where S does not divide the
    DDPM length that grid has one entry more, e.g. 8 for S = 7, and all of them are run, as ``sample(S=7)`` runs them), ``eta``, the
    guidance scale, ``t_start`` (None: the whole schedule; else only its entries t_start - 1 .. 0 are run, as
    ``DDIMSampler.decode(t_start=...)`` does) and the DPM-Solver++ ``order``."""
    steps: int = 50
    eta: float = 0.0
    guidance: float = 1.0
    t_start: Optional[int] = None
    order: int = 2

    def __post_init__(self):
        if not isinstance(self.steps, (int, np.integer)) or not 1 <= int(self.steps) <= MAX_STEPS:
            raise ValueError(f'SampleSpec: steps must be an integer in 1..{MAX_STEPS}, got {self.steps!r}')
        if not float(self.eta) >= 0.0:
            raise ValueError(f'SampleSpec: eta must be >= 0, got {self.eta!r}')
        if not np.isfinite(float(self.guidance)):
            raise ValueError(f'SampleSpec: guidance must be finite, got {self.guidance!r}')
        if self.t_start is not None and not 1 <= int(self.t_start) <= int(self.steps):
            raise ValueError(f'SampleSpec: t_start must lie in 1..steps ({self.steps}), got {self.t_start!r}')
        if self.order not in (1, 2, 3):
            raise ValueError(f'SampleSpec: order must be 1, 2 or 3, got {self.order!r}')


@dataclass
class RowTables:
    """What ``MkdEngine.sample_rows`` takes per sample (mkd_sample_row): float32 tables, entry n - 1 executed first"""
    timesteps: np.ndarray
    alphas: np.ndarray
    alphas_prev: np.ndarray
    sqrt_one_minus_alphas: np.ndarray
    sigmas: Optional[np.ndarray] = None
    dpm: Optional[np.ndarray] = None
    cfg_scale: float = 1.0

    @property
    def n(self) -> int:
        return len(self.timesteps)


def ddim_tables(alphas_cumprod, steps: int, eta: float = 0.0, ddpm_num_timesteps: Optional[int] = None):
    """(timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, sigmas) of ``DDIMSampler.make_schedule(steps, ddim_eta=eta)`` as float32
    arrays, from the functions of schedule.py.  Nothing is registered anywhere: a sampler's buffers are not touched."""
    if isinstance(alphas_cumprod, torch.Tensor):
        alphas_cumprod = alphas_cumprod.detach().cpu().to(torch.float32).numpy()
    acn = np.asarray(alphas_cumprod, dtype=np.float32)
    total = acn.shape[0] if ddpm_num_timesteps is None else int(ddpm_num_timesteps)
    if acn.shape[0] != total:
        raise ValueError('alphas have to be defined for each timestep')
    ts = make_ddim_timesteps('uniform', int(steps), total)
    sig, a, ap = make_ddim_sampling_parameters(acn, ts, float(eta))
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    return np.asarray(ts, dtype=np.int64), f32(a), f32(ap), f32(np.sqrt(1.0 - a)), f32(sig)


def build_rows(specs: Sequence[SampleSpec], alphas_cumprod, solver: str = 'ddim', ddpm_num_timesteps: Optional[int] = None) -> List[RowTables]:
    """One ``RowTables`` per spec.  'ddim': the tables of ``DDIMSampler.make_schedule(spec.steps, ddim_eta=spec.eta)`` cut to
    ``t_start`` entries where that is given; 'dpmpp': the same grid (eta must be 0) and ``dpmpp_table`` of the cut tables at ``spec.order``, which is what
    ``DPMSolverSampler`` runs.  The guidance scale rides along."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be 'ddim' or 'dpmpp', got {solver!r}")
    specs = list(specs)
    if not specs:
        raise ValueError('build_rows: one SampleSpec per sample is needed')
    rows = []
    for b, sp in enumerate(specs):
        if not isinstance(sp, SampleSpec):
            raise TypeError(f'build_rows: specs[{b}] is not a SampleSpec')
        if solver == 'dpmpp' and float(sp.eta) != 0.0:
            raise ValueError(f'build_rows: specs[{b}] has eta = {sp.eta}, DPM-Solver++ is deterministic')
        ts, a, ap, s1, sg = ddim_tables(alphas_cumprod, sp.steps, sp.eta if solver == 'ddim' else 0.0, ddpm_num_timesteps)
        n = len(ts) if sp.t_start is None else int(sp.t_start)          # (every entry of the grid, as the uniform samplers run it)
        row = RowTables(ts[:n], a[:n], ap[:n], s1[:n], cfg_scale=float(sp.guidance))
        if solver == 'ddim':
            row.sigmas = sg[:n] if float(np.abs(sg[:n]).max()) != 0.0 else None
        else:
            from .engine import dpmpp_table          # (host only; the floats the in-library loop uses)
            row.dpm = dpmpp_table(row.alphas, row.alphas_prev, int(sp.order), True)[0]
        rows.append(row)
    return rows


def start_rows(t_starts, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, cfg_scale: float = 1.0, dpm_order: Optional[int] = None) -> List[RowTables]:
    """Per-sample start points on ONE schedule (``DDIMSampler.decode`` / ``MKDDIMSampler.reconstruct`` with a sequence ``t_start``):
    sample b runs entries t_start_b - 1 .. 0 of the given tables.  ``dpm_order``: DPM-Solver++ rows at that order instead."""
    ts = np.asarray(timesteps, dtype=np.int64)
    a, ap, s1 = (np.asarray([float(v) for v in t], dtype=np.float32) for t in (alphas, alphas_prev, sqrt_one_minus_alphas))
    starts = [int(v) for v in torch.as_tensor(t_starts).reshape(-1).tolist()]
    if not starts:
        raise ValueError('t_start: one start point per sample is needed')
    rows = []
    for b, n in enumerate(starts):
        if not 1 <= n <= len(ts):
            raise ValueError(f't_start[{b}] = {n} lies outside 1..{len(ts)} schedule steps')
        row = RowTables(ts[:n], a[:n], ap[:n], s1[:n], cfg_scale=float(cfg_scale))
        if dpm_order is not None:
            from .engine import dpmpp_table
            row.dpm = dpmpp_table(row.alphas, row.alphas_prev, int(dpm_order), True)[0]
        rows.append(row)
    return rows


def guided(rows: Sequence[RowTables]) -> bool:
    """the prepared batch must be doubled ([uncond; cond]) exactly when some sample's scale is not 1"""
    return any(float(r.cfg_scale) != 1.0 for r in rows)


def draw_plan(rows: Sequence[RowTables]) -> List[bool]:
    """The host draw order of eta > 0: entry k tells whether executed step k draws.  One draw of the full batch shape is taken for
    step k when some ACTIVE sample (k < n_b) has a non-zero sigma in its entry n_b - 1 - k."""
    s_max = max(r.n for r in rows)
    plan = []
    for k in range(s_max):
        plan.append(any(r.sigmas is not None and k < r.n and float(r.sigmas[r.n - 1 - k]) != 0.0 for r in rows))
    return plan


def draw_noise(rows: Sequence[RowTables], shape, device='cpu') -> Optional[torch.Tensor]:
    """[S_max, *shape] noise of a per-sample call, or None when no step draws: for each executed step in order one ``torch.randn`` of
    the full batch shape from the default generator where ``draw_plan`` says so, zeros elsewhere (those rows are never read)."""
    plan = draw_plan(rows)
    if not any(plan):
        return None
    return torch.stack([torch.randn(tuple(shape), device=device) if d else torch.zeros(tuple(shape), device=device) for d in plan])


def step_map(rows: Sequence[RowTables]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[int]]:
    """Restatement of the step table's bookkeeping (mkd_step_table): ``(entry [S_max, B], active [S_max, B], temb_row [S_max, B],
    distinct timesteps)``.  entry = n_b - 1 - k while active, 0 afterwards (a finished sample is evaluated at the timestep of its entry
    0); the time-embedding table has one row per distinct timestep in first-seen order, steps outer, samples inner."""
    B, s_max = len(rows), max(r.n for r in rows)
    entry = np.zeros((s_max, B), dtype=np.int64)
    active = np.zeros((s_max, B), dtype=bool)
    temb = np.zeros((s_max, B), dtype=np.int64)
    distinct: List[int] = []
    for k in range(s_max):
        for b, r in enumerate(rows):
            active[k, b] = k < r.n
            entry[k, b] = r.n - 1 - k if active[k, b] else 0
            t = int(r.timesteps[entry[k, b]])
            if t not in distinct:
                distinct.append(t)
            temb[k, b] = distinct.index(t)
    return entry, active, temb, distinct
