"""Restatement of the temporal makeup filter (include/mkd.h mkd_temporal_diff; test infrastructure only): numpy float32, one numpy
operation per rounding, in the header's order; the window sum in int64 (exact).  ``step`` is one face of one frame step, ``run`` a
clip of one face, ``pools_step`` the call itself with its pools and slots."""
import numpy as np

F = np.float32


def luma(s01: np.ndarray) -> np.ndarray:
    """s01 float32 [3,S,S] -> int64 [S,S]: 77 R + 150 G + 29 B of the bytes clamp(rint(s01 * 255), 0, 255)"""
    gb = np.clip(np.rint(np.asarray(s01, F) * F(255.0)), F(0.0), F(255.0)).astype(np.int64)
    y = 77 * gb[0] + 150 * gb[1] + 29 * gb[2]
    assert int(y.max()) <= 65280
    return y


def diff(t: np.ndarray, s01: np.ndarray) -> np.ndarray:
    d = ((np.asarray(t, F) + F(1.0)) * F(0.5)) - np.asarray(s01, F)
    assert d.dtype == F
    return d


def window_sum(a: np.ndarray, radius: int) -> np.ndarray:
    """int64 [S,S] -> the sum over the (2 R + 1)^2 window with replicated edges"""
    S = a.shape[0]
    p = np.pad(a, radius, mode='edge')
    out = np.zeros_like(a)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out += p[dy:dy + S, dx:dx + S]
    return out


def gain(y: np.ndarray, y_in: np.ndarray, beta: float, tau: float, radius: int) -> np.ndarray:
    """k float32 [S,S] of a face with a previous frame: y int64 [S,S] of this frame, y_in float32 [S,S] of the previous one"""
    n = (2 * radius + 1) ** 2
    A = window_sum(np.abs(y - np.asarray(y_in, F).astype(np.int64)), radius)
    inv = F(1.0) / ((F(256.0) * F(tau)) * F(n))
    q = A.astype(F) * inv
    c = F(1.0) / (F(1.0) + q * q)
    k = F(beta) * c
    assert k.dtype == F
    return k


def step(t, s01, D_in=None, Y_in=None, beta: float = 0.8, tau: float = 4.0, radius: int = 1):
    """one face: t / s01 float32 [3,S,S], D_in [3,S,S] / Y_in [S,S] float32 or None (no previous frame) -> (t_out, D_out, Y_out)"""
    t, s01 = np.asarray(t, F), np.asarray(s01, F)
    y = luma(s01)
    d = diff(t, s01)
    if D_in is None:
        return t.copy(), d, y.astype(F)
    k = gain(y, Y_in, beta, tau, radius)
    D = d + k[None] * (np.asarray(D_in, F) - d)
    t_out = ((s01 + D) * F(2.0)) - F(1.0)
    assert D.dtype == F and t_out.dtype == F
    return t_out, D, y.astype(F)


def run(ts, s01s, beta: float = 0.8, tau: float = 4.0, radius: int = 1):
    """a clip of one face: lists of t / s01 per frame -> (list of t_out, list of D)"""
    D = Y = None
    outs, Ds = [], []
    for t, s in zip(ts, s01s):
        o, D, Y = step(t, s, D, Y, beta, tau, radius)
        outs.append(o)
        Ds.append(D)
    return outs, Ds


def pools_step(t, s01, D_in, Y_in, slot_in, D_out, Y_out, slot_out, beta: float, tau: float, radius: int):
    """the call: t / s01 [n,3,S,S]; pools D [pool,3,S,S], Y [pool,S,S]; slots int [n] -> t_out [n,3,S,S]; D_out / Y_out are written
    in place in the slots named, everything else of them stays"""
    t_out = np.empty_like(np.asarray(t, F))
    for b in range(t.shape[0]):
        si, so = int(slot_in[b]), int(slot_out[b])
        prev = (None, None) if si < 0 else (D_in[si], Y_in[si])
        t_out[b], D_out[so], Y_out[so] = step(t[b], s01[b], prev[0], prev[1], beta, tau, radius)
    return t_out
