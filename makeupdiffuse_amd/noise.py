"""Counter-based noise on the device (mkd_noise_fill; include/mkd.h has the definition): element e of row r of sample b is a pure
function of (seed_b, sub_b, stream, r, e).  No generator state exists: the torch generators are neither read nor advanced, and what a
sample gets does not depend on the batch it is in, on its position there or on what ran before.

``normal`` is the draw, ``as_seeds`` the one place seeds are validated; ``Seeds`` carries one seed (and optionally one sub-stream) per
sample through the samplers and the model, which take it wherever they take ``seeds=``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as mlib

__all__ = ['STREAM_START', 'STREAM_ETA', 'STREAM_BLEND', 'STREAM_POSTERIOR', 'STREAM_TEACHER', 'STREAM_USER', 'Seeds', 'as_seeds',
           'normal', 'words', 'teacher_timesteps']

# what a draw is for (the `stream_id` of mkd_noise_fill): 5..15 are reserved, STREAM_USER and above are free for callers
STREAM_START = 0          # the start latent x_T (row 0)
STREAM_ETA = 1            # the eta noise of executed step k (row k)
STREAM_BLEND = 2          # the q_sample noise of the masked blend before executed step k (row k); stochastic_encode: row 0
STREAM_POSTERIOR = 3      # the first-stage posterior sample (row 0)
STREAM_TEACHER = 4        # the q_sample noise of log_results' sample_ddmp row (row 0)
STREAM_USER = 16

_U64 = 1 << 64
_U32 = 1 << 32


def _ints(v, what) -> list:
    if isinstance(v, torch.Tensor):
        if v.dim() != 1 or v.is_floating_point() or v.dtype == torch.bool:
            raise ValueError(f'{what} must be a 1-D integer tensor, got {tuple(v.shape)} {v.dtype}')
        v = v.tolist()
    elif isinstance(v, np.ndarray):
        if v.ndim != 1 or v.dtype.kind not in 'iu':
            raise ValueError(f'{what} must be a 1-D integer array, got {v.shape} {v.dtype}')
        v = v.tolist()
    out = []
    for x in v:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError(f'{what} must be integers, got {x!r}')
        out.append(int(x))
    return out


@dataclass(frozen=True)
class Seeds:
    """One 64-bit seed per sample and, optionally, one 32-bit sub-stream each (None: all 0).  Built by ``as_seeds``."""
    seeds: Tuple[int, ...]
    subs: Optional[Tuple[int, ...]] = None

    def __len__(self) -> int:
        return len(self.seeds)

    def take(self, idx: Sequence[int]) -> 'Seeds':
        """the samples ``idx`` of this batch, in that order (a sub-batch keeps every sample's noise)"""
        idx = [int(i) for i in idx]
        return Seeds(tuple(self.seeds[i] for i in idx), None if self.subs is None else tuple(self.subs[i] for i in idx))


def as_seeds(seed_or_seqs, B: int, subs=None) -> Seeds:
    """Seeds of a batch of ``B``: an int s means s, s + 1, ..., s + B - 1; a sequence (list, tuple, 1-D integer array or tensor) gives one
    seed per sample; a ``Seeds`` of length B is taken as it is.  Every seed lies in 0 .. 2^64 - 1, every sub in 0 .. 2^32 - 1;
    ``subs`` (one per sample, or None) replaces the sub-streams.  ValueError otherwise."""
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or int(B) < 1:
        raise ValueError(f'as_seeds: the batch must be an integer >= 1, got {B!r}')
    B = int(B)
    if isinstance(seed_or_seqs, Seeds):
        seeds, own = list(seed_or_seqs.seeds), seed_or_seqs.subs
    elif isinstance(seed_or_seqs, (bool, np.bool_)) or seed_or_seqs is None:
        raise ValueError(f'as_seeds: a seed is an integer or a sequence of integers, got {seed_or_seqs!r}')
    elif isinstance(seed_or_seqs, (int, np.integer)):
        seeds, own = [int(seed_or_seqs) + i for i in range(B)], None
    elif isinstance(seed_or_seqs, (list, tuple, np.ndarray, torch.Tensor)):
        seeds, own = _ints(seed_or_seqs, 'as_seeds: seeds'), None
    else:
        raise ValueError(f'as_seeds: a seed is an integer or a sequence of integers, got {seed_or_seqs!r}')
    if len(seeds) != B:
        raise ValueError(f'as_seeds: {len(seeds)} seeds for a batch of {B}')
    for s in seeds:
        if not 0 <= s < _U64:
            raise ValueError(f'as_seeds: a seed must lie in 0 .. 2^64 - 1, got {s}')
    if subs is not None:
        if isinstance(subs, (bool, np.bool_)):
            raise ValueError(f'as_seeds: subs must be integers, got {subs!r}')
        own = [int(subs)] * B if isinstance(subs, (int, np.integer)) else _ints(subs, 'as_seeds: subs')
    if own is not None:
        own = [int(v) for v in own]
        if len(own) != B:
            raise ValueError(f'as_seeds: {len(own)} subs for a batch of {B}')
        for v in own:
            if not 0 <= v < _U32:
                raise ValueError(f'as_seeds: a sub must lie in 0 .. 2^32 - 1, got {v}')
    return Seeds(tuple(seeds), None if own is None else tuple(own))


def teacher_timesteps(seeds: Seeds, t_min: int, T: int) -> list:
    """The timestep t_b in [t_min, T) of log_results' sample_ddmp row for every sample of ``seeds``: a pure function of (seed_b, sub_b),
    computed on the host in 64-bit integer arithmetic (the splitmix64 finaliser):
        z = (seed + 0x9E3779B97F4A7C15 (sub + 1)) mod 2^64;  z = ((z ^ (z >> 30)) 0xBF58476D1CE4E5B9) mod 2^64;
        z = ((z ^ (z >> 27)) 0x94D049BB133111EB) mod 2^64;  z = z ^ (z >> 31);  t = t_min + z mod (T - t_min)"""
    t_min, T = int(t_min), int(T)
    if not 0 <= t_min < T:
        raise ValueError(f'teacher_t_min must lie in 0 .. {T - 1}, got {t_min}')
    out = []
    for b, seed in enumerate(seeds.seeds):
        sub = 0 if seeds.subs is None else seeds.subs[b]
        z = (seed + 0x9E3779B97F4A7C15 * (sub + 1)) % _U64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % _U64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % _U64
        z ^= z >> 31
        out.append(t_min + z % (T - t_min))
    return out


def _fill(seeds, shape, stream, rows, row0, subs, device, kind):
    shape = tuple(int(v) for v in shape)
    if not shape or any(v < 1 for v in shape):
        raise ValueError(f'noise: the per-sample shape must be non-empty with positive sizes, got {shape}')
    for name, v in (('stream', stream), ('row0', row0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < _U32:
            raise ValueError(f'noise: {name} must be an integer in 0 .. 2^32 - 1, got {v!r}')
    if rows is not None and (isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or int(rows) < 1):
        raise ValueError(f'noise: rows must be None or an integer >= 1, got {rows!r}')
    if isinstance(seeds, Seeds):
        sd = seeds if subs is None else as_seeds(seeds, len(seeds), subs)
    elif isinstance(seeds, (int, np.integer)) and not isinstance(seeds, bool):
        raise ValueError('noise: one seed per sample is needed (as_seeds(seed, B) spells a start seed out)')
    else:
        sd = as_seeds(seeds, len(seeds) if hasattr(seeds, '__len__') else -1, subs)
    B, n_rows = len(sd), 1 if rows is None else int(rows)
    if int(row0) + n_rows - 1 >= _U32:
        raise ValueError(f'noise: row0 + rows - 1 must fit 32 bits, got {int(row0) + n_rows - 1}')
    device = torch.device(device)
    if device.type != 'cuda':
        raise mlib.MkdError(f'noise is drawn on the device (mkd_noise_fill): device {device} is not a HIP device, and there is no CPU path')
    n = int(np.prod(shape, dtype=np.int64))
    lib = mlib.load()
    # the int64 carrier of a uint64: the bits
    s_dev = torch.tensor([s - _U64 if s >= (1 << 63) else s for s in sd.seeds], dtype=torch.int64, device=device)
    u_dev = None if sd.subs is None else torch.tensor([v - _U32 if v >= (1 << 31) else v for v in sd.subs], dtype=torch.int32, device=device)
    out = torch.empty((n_rows, B) + shape, dtype=torch.float32 if kind == 0 else torch.int32, device=device)
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device).cuda_stream
        mlib.check(lib.mkd_noise_fill(C.c_void_p(s_dev.data_ptr()), C.c_void_p(None if u_dev is None else u_dev.data_ptr()), B, int(stream),
                                      int(row0), n_rows, n, int(kind), C.c_void_p(out.data_ptr()), C.c_void_p(st)), 'mkd_noise_fill')
    # (s_dev / u_dev go back to the caching allocator of the stream the kernel was enqueued on: stream order keeps them valid)
    return out if rows is not None else out[0]


def normal(seeds, shape, *, stream, rows=None, row0=0, subs=None, device) -> torch.Tensor:
    """Standard normals, fp32 ``[B, *shape]`` on ``device``, or ``[rows, B, *shape]`` when ``rows`` is given: sample b's values are those
    of (seeds[b], subs[b], stream, row) with row = ``row0`` (+ i for row i), whatever else is in the batch.  ``seeds``: a sequence of
    B integers or a ``Seeds``; ``subs``: None (all 0, or the ``Seeds``' own), one integer for all, or one per sample.  One launch;
    no torch generator is touched.  MkdError off the device."""
    return _fill(seeds, shape, stream, rows, row0, subs, device, 0)


def words(seeds, shape, *, stream, rows=None, row0=0, subs=None, device) -> torch.Tensor:
    """The raw Philox words under ``normal``'s values (kind 1 of mkd_noise_fill; tests): int32 tensors holding the uint32 bits."""
    return _fill(seeds, shape, stream, rows, row0, subs, device, 1)
