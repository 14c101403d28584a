"""Restatement of the block-matched motion in front of the temporal makeup filter (include/mkd.h mkd_motion_warp; test infrastructure
only): integer luminance (tests/video_ref.py luma), a plain double loop over the candidates, the explicit lexicographic key
(cost, |vy| + |vx|, vy, vx) and the copy of the previous state through the chosen vectors.  ``vectors`` is one face, ``warp`` its copy,
``pools_warp`` the call itself with its pools and slots, ``frame_step`` one filtered frame step (the warp, then video_ref.pools_step on
the warped pools)."""
import numpy as np

import video_ref as vr


def clamp_idx(S: int, v: int) -> np.ndarray:
    """the indices clamp(p + v, 0, S - 1) of p = 0 .. S - 1"""
    return np.clip(np.arange(S) + int(v), 0, S - 1)


def vectors(y: np.ndarray, yp: np.ndarray, search: int, block: int, penalty: int) -> np.ndarray:
    """y int [S,S] of this frame, yp int [S,S] of the previous one -> int32 [nb, nb, 2] = (vy, vx) per block"""
    y, yp = np.asarray(y, np.int64), np.asarray(yp, np.int64)
    S = y.shape[0]
    nb = -(-S // block)
    out = np.zeros((nb, nb, 2), np.int32)
    for by in range(nb):
        for bx in range(nb):
            ys, xs = slice(by * block, min(S, (by + 1) * block)), slice(bx * block, min(S, (bx + 1) * block))
            N = (ys.stop - ys.start) * (xs.stop - xs.start)
            best = None
            for vy in range(-search, search + 1):
                for vx in range(-search, search + 1):
                    shifted = yp[clamp_idx(S, vy)[ys]][:, clamp_idx(S, vx)[xs]]
                    sad = int(np.abs(y[ys, xs] - shifted).sum())
                    cost = sad + penalty * N * (abs(vy) + abs(vx))
                    assert cost < 2 ** 31
                    key = (cost, abs(vy) + abs(vx), vy, vx)
                    if best is None or key < best:
                        best = key
            out[by, bx] = best[2:]
    return out


def warp(a: np.ndarray, vec: np.ndarray, block: int) -> np.ndarray:
    """a [..., S, S] -> the same shape: pixel p of block (by, bx) takes a[..., clamp(p + vec[by, bx])] (the bits)"""
    S = a.shape[-1]
    out = np.empty_like(a)
    for by in range(vec.shape[0]):
        for bx in range(vec.shape[1]):
            ys, xs = slice(by * block, min(S, (by + 1) * block)), slice(bx * block, min(S, (bx + 1) * block))
            vy, vx = (int(v) for v in vec[by, bx])
            out[..., ys, xs] = a[..., clamp_idx(S, vy)[ys], :][..., clamp_idx(S, vx)[xs]]
    return out


def pools_warp(s01, D_in, Y_in, slot_in, D_w, Y_w, search: int, block: int, penalty: int) -> np.ndarray:
    """the call: s01 [n,3,S,S]; pools D [pool,3,S,S], Y [pool,S,S]; slot_in int [n] -> the vectors int32 [n, nb, nb, 2]; D_w / Y_w are
    written in place in the slots named (the slot read is the slot written), everything else of them stays; a face with slot -1 has
    zero vectors and touches no pool"""
    n, S = s01.shape[0], s01.shape[2]
    nb = -(-S // block)
    vec = np.zeros((n, nb, nb, 2), np.int32)
    for b in range(n):
        si = int(slot_in[b])
        if si < 0:
            continue
        vec[b] = vectors(vr.luma(s01[b]), np.asarray(Y_in[si], np.float32).astype(np.int64), search, block, penalty)
        D_w[si] = warp(D_in[si], vec[b], block)
        Y_w[si] = warp(Y_in[si], vec[b], block)
    return vec


def frame_step(t, s01, D_in, Y_in, slot_in, D_w, Y_w, D_out, Y_out, slot_out, filt, ms):
    """one filtered frame step with motion: filt = (beta, tau, radius), ms = (search, block, penalty) or None (no motion: the _in pools
    are read as they are) -> (t_out [n,3,S,S], the vectors or None)"""
    vec = None
    if ms is not None:
        vec = pools_warp(s01, D_in, Y_in, slot_in, D_w, Y_w, *ms)
        D_in, Y_in = D_w, Y_w
    return vr.pools_step(t, s01, D_in, Y_in, slot_in, D_out, Y_out, slot_out, *filt), vec
