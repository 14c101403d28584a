"""numpy restatement of mkd_label_components (include/mkd.h): the 8-connected components of the pixels whose label is in a class
set.  Row runs, a union-find over the runs that touch in adjacent rows (diagonally too), then ids (smallest linear index), areas,
inclusive boxes, the table's order (area descending, ties by id ascending) and its fill rows.  Everything is an integer.  No loop
runs per pixel: the union-find hooks and compresses whole arrays of runs (a 1024 x 1024 map takes well under a second)."""
import numpy as np

INT_MAX = 2 ** 31 - 1
FILL_ROW = (-1, 0, INT_MAX, -1, INT_MAX, -1)


def in_mask(labels: np.ndarray, classes) -> np.ndarray:
    """a pixel is in when its label l < 64 is one of ``classes`` (labels >= 64 never match)"""
    lut = np.zeros(256, bool)
    for c in classes:
        assert 0 <= int(c) < 64
        lut[int(c)] = True
    return lut[np.asarray(labels, np.uint8)]


def row_runs(mask: np.ndarray):
    """(row, first column, last column) of every maximal horizontal run of True, in row-major order"""
    H, W = mask.shape
    p = np.zeros((H, W + 2), np.int8)
    p[:, 1:-1] = mask
    d = np.diff(p, axis=1)                       # [H, W + 1]: +1 at a run's first column, -1 one past its last
    ry, rs = np.nonzero(d == 1)
    _, re = np.nonzero(d == -1)
    return ry.astype(np.int64), rs.astype(np.int64), re.astype(np.int64) - 1


def run_edges(ry, rs, re, W: int):
    """pairs (a in row y, b in row y + 1) of runs that touch under 8-connectivity: a.first <= b.last + 1 and b.first <= a.last + 1.
    Runs of a row are disjoint and sorted, so the partners of b are a contiguous range found by two binary searches"""
    M = W + 4
    key_end, key_start = ry * M + re + 1, ry * M + rs + 1
    lo = np.searchsorted(key_end, (ry - 1) * M + rs, side='left')               # first run of the row above with last + 1 >= first
    hi = np.searchsorted(key_start, (ry - 1) * M + re + 2, side='right')        # one past the last with first <= last + 1
    n = np.maximum(hi - lo, 0)
    n[ry == 0] = 0
    b = np.repeat(np.arange(len(ry)), n)
    a = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    return a, b


def union_find(n: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """root[i] = the smallest index of i's set after uniting a[k] with b[k] for every k"""
    parent = np.arange(n)
    while True:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not live.any():
            return parent
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))             # hook the larger root under the smaller
        while True:                                                               # compress: every entry points at a root
            g = parent[parent]
            if np.array_equal(g, parent):
                break
            parent = g


def components_of_mask(mask: np.ndarray):
    """ids int32 [H,W] (-1 outside) and, per component in id order, (id, area, r0, r1, c0, c1) int64 [n, 6]"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    ids = np.full((H, W), -1, np.int32)
    ry, rs, re = row_runs(mask)
    if len(ry) == 0:
        return ids, np.zeros((0, 6), np.int64)
    a, b = run_edges(ry, rs, re, W)
    root = union_find(len(ry), a, b)
    roots, comp = np.unique(root, return_inverse=True)                # runs are in row-major order: a root run holds the smallest pixel
    cid = ry[roots] * W + rs[roots]
    length = re - rs + 1
    n = len(roots)
    area = np.bincount(comp, weights=length, minlength=n).astype(np.int64)
    r0, r1 = np.full(n, INT_MAX, np.int64), np.full(n, -1, np.int64)
    c0, c1 = np.full(n, INT_MAX, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(r0, comp, ry)
    np.maximum.at(r1, comp, ry)
    np.minimum.at(c0, comp, rs)
    np.maximum.at(c1, comp, re)
    ids.reshape(-1)[np.flatnonzero(mask)] = np.repeat(cid[comp], length)          # in-pixels in row-major order = the runs in order
    return ids, np.stack((cid, area, r0, r1, c0, c1), 1)


def table_of(comps: np.ndarray, min_area: int, max_out: int):
    """(table int32 [max_out, 6], count) from the rows of components_of_mask"""
    keep = comps[comps[:, 1] >= min_area]
    keep = keep[np.lexsort((keep[:, 0], -keep[:, 1]))]
    table = np.tile(np.array(FILL_ROW, np.int64), (max_out, 1))
    k = min(len(keep), max_out)
    table[:k] = keep[:k]
    return table.astype(np.int32), len(keep)


def label_components(labels: np.ndarray, classes, min_area: int = 1, max_out: int = 16):
    """labels uint8 [B,H,W] or [H,W] -> (table int32 [B,max_out,6], count int32 [B], ids int32 [B,H,W]): the library's outputs"""
    labels = np.asarray(labels, np.uint8)
    if labels.ndim == 2:
        labels = labels[None]
    tables, counts, idss = [], [], []
    for lab in labels:
        ids, comps = components_of_mask(in_mask(lab, classes))
        t, c = table_of(comps, min_area, max_out)
        tables.append(t)
        counts.append(c)
        idss.append(ids)
    return np.stack(tables), np.array(counts, np.int32), np.stack(idss)
