"""Restatement of the owner calls (include/mkd.h mkd_owner_map, mkd_owner_weights, mkd_paste_photo_weighted; test infrastructure
only): the nearest table component of every pixel by brute force over all seeds with the key (d^2, rank), the same from one
scipy.ndimage.distance_transform_edt per rank, the window fractions in integers with one float32 division, and the weighted paste on
tests/photo_ref.py's functions with one numpy float32 operation per rounding."""
import numpy as np

import photo_ref as pr

NO_OWNER = 255
NO_DIST = 2 ** 31 - 1


def seed_ranks(ids: np.ndarray, table_ids) -> np.ndarray:
    """ids int [H,W] (-1: no component), table_ids the id column of one image's table -> int [H,W]: the rank of every seed pixel,
    -1 elsewhere.  Rows with id < 0 hold nothing; of rows that repeat an id the lowest counts."""
    rank = np.full(ids.shape, -1, np.int64)
    for r in reversed(range(len(table_ids))):
        if table_ids[r] >= 0:
            rank[ids == table_ids[r]] = r
    return rank


def owner_brute(ids: np.ndarray, table_ids):
    """-> (owner uint8 [H,W], dist2 int32 [H,W]): the minimum over ALL seeds of the key d^2 * 256 + rank"""
    H, W = ids.shape
    rank = seed_ranks(ids, table_ids)
    sy, sx = np.nonzero(rank >= 0)
    if len(sy) == 0:
        return np.full((H, W), NO_OWNER, np.uint8), np.full((H, W), NO_DIST, np.int32)
    sr = rank[sy, sx]
    yy, xx = np.mgrid[:H, :W]
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    for v, u, r in zip(sy.tolist(), sx.tolist(), sr.tolist()):
        np.minimum(best, ((yy - v) ** 2 + (xx - u) ** 2) * 256 + r, out=best)
    return (best % 256).astype(np.uint8), (best // 256).astype(np.int32)


def owner_edt(ids: np.ndarray, table_ids):
    """the same from one exact Euclidean distance transform per rank, squared and rounded; the lowest rank on equality"""
    from scipy import ndimage
    H, W = ids.shape
    rank = seed_ranks(ids, table_ids)
    owner, dist = np.full((H, W), NO_OWNER, np.uint8), np.full((H, W), NO_DIST, np.int64)
    for r in range(len(table_ids)):
        if not (rank == r).any():
            continue
        d2 = np.rint(ndimage.distance_transform_edt(rank != r) ** 2).astype(np.int64)
        closer = d2 < dist                                   # strictly: an earlier (lower) rank keeps a tie
        owner[closer], dist[closer] = r, d2[closer]
    return owner, dist.astype(np.int32)


def ids_of_seeds(H: int, W: int, seeds):
    """seeds [(y, x), ...] or [[(y, x), ...], ...] (one list of pixels per component) -> (ids int32 [H,W], ids of the components in
    the order given): a component's id is the smallest linear index of its pixels, as mkd_label_components defines it"""
    ids = np.full((H, W), -1, np.int32)
    out = []
    for comp in seeds:
        comp = [comp] if isinstance(comp[0], int) else list(comp)
        cid = min(y * W + x for y, x in comp)
        for y, x in comp:
            ids[y, x] = cid
        out.append(cid)
    return ids, out


def tie_layouts():
    """[(name, ids [H,W], table ids)]: two components at equal distance from some pixels, each layout also with the table's two rows
    swapped -- the owner of the tied pixels must be rank 0 both times, so the rank decides and not the position"""
    out = []
    for name, H, W, a, b in (('mirrored about a column', 5, 9, (2, 1), (2, 7)),          # column 4 ties, through different columns
                             ('above and below in one column', 9, 3, (1, 1), (7, 1)),    # row 4 of column 1: the up/down tie of the column pass
                             ('a diagonal pair', 7, 7, (1, 1), (5, 5))):                 # the anti-diagonal ties
        ids, (ia, ib) = ids_of_seeds(H, W, [a, b])
        out.append((name, ids, [ia, ib]))
        out.append((name + ', ranks swapped', ids, [ib, ia]))
    return out


def weights(owner: np.ndarray, rank: int, rho: int) -> np.ndarray:
    """owner uint8 [H,W] -> float32 [H,W]: float(S) / float((2 rho + 1)^2), S the window's pixels (indices clamped to the edge) that
    ``rank`` owns"""
    H, W = owner.shape
    flag = np.pad((owner == rank).astype(np.int64), rho, mode='edge')
    S = np.zeros((H, W), np.int64)
    for dy in range(2 * rho + 1):
        for dx in range(2 * rho + 1):
            S += flag[dy:dy + H, dx:dx + W]
    out = S.astype(np.float32) / np.float32((2 * rho + 1) ** 2)
    assert out.dtype == np.float32
    return out


def _lerp(a, b, w):
    return a + w * (b - a)


def weight_at_photo(w: np.ndarray, H: int, W: int) -> np.ndarray:
    """w float32 [wh,ww] over the whole H x W photo -> float32 [H,W]: the paste's half-pixel, clamp-to-edge bilinear sample"""
    w = np.asarray(w, np.float32)
    xa, xb, ux = pr._axis(W, w.shape[1])
    ya, yb, uy = pr._axis(H, w.shape[0])
    ux, uy = ux[None, :], uy[:, None]
    g = _lerp(_lerp(w[ya][:, xa], w[ya][:, xb], ux), _lerp(w[yb][:, xa], w[yb][:, xb], ux), uy)
    assert g.dtype == np.float32
    return g


def paste_weighted(photo: np.ndarray, box, t: np.ndarray, s01: np.ndarray, rho: int, w: np.ndarray) -> np.ndarray:
    """photo_ref.paste with the feather weight multiplied by the photo-wide weight plane w [wh,ww]"""
    H, W = photo.shape[:2]
    x0, y0, bw, bh = box
    S = t.shape[-1]
    t, s01 = np.asarray(t, np.float32), np.asarray(s01, np.float32)
    r = (t + np.float32(1.0)) * np.float32(0.5)
    d = (r - s01) * np.float32(255.0)
    xa, xb, wx = pr._axis(bw, S)
    ya, yb, wy = pr._axis(bh, S)
    wx, wy = wx[None, None, :], wy[None, :, None]
    top = _lerp(d[:, ya][:, :, xa], d[:, ya][:, :, xb], wx)
    bot = _lerp(d[:, yb][:, :, xa], d[:, yb][:, :, xb], wx)
    u = _lerp(top, bot, wy)
    a = pr.feather_alpha(H, W, box, rho) * weight_at_photo(w, H, W)[y0:y0 + bh, x0:x0 + bw]
    region = photo[y0:y0 + bh, x0:x0 + bw].transpose(2, 0, 1).astype(np.float32)
    o = region + a[None] * u
    assert o.dtype == np.float32
    o = np.clip(np.rint(o), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    out = photo.copy()
    out[y0:y0 + bh, x0:x0 + bw] = o.transpose(1, 2, 0)
    return out
