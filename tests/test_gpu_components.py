"""-m gpu: mkd_label_components against the numpy restatement (tests/components_ref.py), exactly: table, count and ids_out.  Every case
runs the call twice, into differently poisoned outputs and scratch, and the two runs must give the same bytes.  The shapes sit at the
seams of the kernels' 32 x 32 tile, not at the workload's size."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_ref as cr
from makeupdiffuse_amd import components
from makeupdiffuse_amd import lib as mlib

pytestmark = pytest.mark.gpu

T = 32          # CC_T of kernels_components.hip
DEV = 'cuda'


def P(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def device_run(labels: np.ndarray, classes, min_area, max_out, poison):
    """one library call with every output and the scratch filled with ``poison`` bytes first -> (table, count, ids) as numpy"""
    lib = mlib.load()
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(DEV)
    B, H, W = lab.shape
    table = torch.full((B, max_out, 6 * 4), poison, device=DEV, dtype=torch.uint8)
    count = torch.full((B, 4), poison, device=DEV, dtype=torch.uint8)
    ids = torch.full((B, H, W * 4), poison, device=DEV, dtype=torch.uint8)
    nbytes = int(lib.mkd_label_components_scratch_bytes(B, H, W))
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.full((nbytes + 256,), poison, device=DEV, dtype=torch.uint8)
    base = (scratch.data_ptr() + 255) & ~255
    rc = lib.mkd_label_components(P(lab), B, H, W, C.c_uint64(components.class_bits(classes)), min_area, max_out, P(table), P(count), P(ids),
                                  C.c_void_p(base), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mkd_last_error()
    torch.cuda.synchronize()
    return (table.cpu().numpy().view(np.int32).reshape(B, max_out, 6), count.cpu().numpy().view(np.int32).reshape(B),
            ids.cpu().numpy().view(np.int32).reshape(B, H, W))


def check(labels, classes=(1,), min_area=1, max_out=16):
    labels = np.asarray(labels, np.uint8)
    if labels.ndim == 2:
        labels = labels[None]
    want = cr.label_components(labels, classes, min_area, max_out)
    one = device_run(labels, classes, min_area, max_out, 0xCD)
    two = device_run(labels, classes, min_area, max_out, 0x3B)
    for name, w, a, b in zip(('table', 'count', 'ids'), want, one, two):
        assert a.tobytes() == b.tobytes(), f'{name}: two runs differ'
        assert np.array_equal(a, w), f'{name}: {int((a != w).sum())} of {a.size} entries differ from the restatement'
    return want


def corners(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    return m


def checkerboard(H, W):
    return ((np.add.outer(np.arange(H), np.arange(W)) & 1) == 0).astype(np.uint8)


def serpentine(H, W):
    """one line, one pixel wide: every second row, joined at alternating ends"""
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def random_map(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


SHAPES = [(1, 1), (1, 70), (70, 1), (T, T), (T + 1, T), (T, T + 1), (T + 1, T + 1), (37, 53), (130, 67), (96, 96)]


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{h}x{w}' for h, w in SHAPES])
def test_basic_patterns_at_the_tile_seams(shape):
    """empty, full, a pixel in each corner, the checkerboard (ONE component under 8-connectivity: a 4-connected merge fails here) and a
    random map, as one batch"""
    H, W = shape
    batch = np.stack([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), corners(H, W), checkerboard(H, W), random_map(H, W, 0.5, H * 1000 + W)])
    table, count, _ = check(batch, max_out=8)
    assert count[0] == 0 and count[1] == 1 and table[1, 0].tolist() == [0, H * W, 0, H - 1, 0, W - 1]
    if min(H, W) > 1:
        assert count[2] == 4 and count[3] == 1 and table[3, 0, 1] == (H * W + 1) // 2


def test_blobs_touching_diagonally_across_a_tile_corner_are_one():
    a = np.zeros((2 * T, 2 * T), np.uint8)
    a[T - 4:T, T - 4:T] = 1
    a[T:T + 4, T:T + 4] = 1          # (T-1, T-1) and (T, T)
    b = np.zeros((2 * T, 2 * T), np.uint8)
    b[T - 4:T, T:T + 4] = 1
    b[T:T + 4, T - 4:T] = 1          # (T-1, T) and (T, T-1)
    table, count, _ = check(np.stack([a, b]))
    assert count.tolist() == [1, 1] and table[0, 0, 1] == 32 and table[1, 0, 1] == 32


def test_blobs_one_pixel_apart_along_a_tile_border_are_two():
    maps = []
    for gap in (T - 1, T):                       # the empty line is the last of a tile, or the first of the next
        v = np.zeros((2 * T, 2 * T + 5), np.uint8)
        v[10:50, gap - 6:gap] = 1
        v[10:50, gap + 1:gap + 7] = 1
        h = np.zeros((2 * T, 2 * T + 5), np.uint8)
        h[gap - 6:gap, 3:60] = 1
        h[gap + 1:gap + 7, 3:60] = 1
        maps += [v, h]
    _, count, _ = check(np.stack(maps))
    assert count.tolist() == [2, 2, 2, 2]


@pytest.mark.parametrize('side', [96, 512])
def test_serpentine_crosses_every_tile_many_times(side):
    m = serpentine(side, side)
    table, count, _ = check(m)
    assert count[0] == 1 and table[0, 0, 0] == 0 and table[0, 0, 1] == int(m.sum())


@pytest.mark.parametrize('density', [0.3, 0.5, 0.6])
def test_random_maps_near_the_percolation_threshold(density):
    _, count, _ = check(random_map(130, 67, density, int(density * 100)), max_out=32)
    assert count[0] > 1


def test_equal_areas_go_by_id_and_missing_rows_are_fill_rows():
    m = np.zeros((70, 75), np.uint8)
    for y, x in ((40, 50), (2, 60), (2, 3), (30, 30), (60, 8)):          # five 3 x 3 squares, one of them across a tile corner
        m[y:y + 3, x:x + 3] = 1
    m[20:25, 20:25] = 1                                                 # and a larger one
    table, count, _ = check(m, max_out=9)
    assert count[0] == 6 and table[0, 0, 1] == 25
    assert table[0, 1:6, 0].tolist() == sorted(table[0, 1:6, 0].tolist()) and (table[0, 1:6, 1] == 9).all()
    assert [r.tolist() for r in table[0, 6:]] == [list(cr.FILL_ROW)] * 3


def test_more_components_than_rows_count_is_not_capped():
    m = random_map(67, 130, 0.15, 7)
    table, count, _ = check(m, max_out=4)
    assert count[0] > 4 and (table[0, :, 0] >= 0).all()
    check(m, max_out=1)
    check(m, max_out=64)


def test_min_area_filters_the_table_but_not_the_ids():
    m = random_map(90, 70, 0.3, 11)
    table, count, ids = check(m, min_area=6, max_out=16)
    all_table, all_count, _ = cr.label_components(m, (1,), 1, 64)
    assert 0 < count[0] < all_count[0] and (table[0, :min(count[0], 16), 1] >= 6).all()
    assert (ids[0] >= 0).sum() == int(m.sum())                          # the small components keep their ids
    check(m, min_area=10 ** 6)                                          # nothing is large enough: count 0, fill rows only


def test_class_subsets_and_labels_past_63():
    g = np.random.default_rng(5)
    m = g.choice(np.array([0, 1, 5, 9, 63, 64, 200, 255], np.uint8), size=(2, 67, 99))
    for classes in ((1, 9), (63,), (0, 5), tuple(range(64))):
        check(m, classes=classes, max_out=8)
    _, count, _ = check(np.full((1, 40, 40), 64, np.uint8), classes=tuple(range(64)))          # label 64 is never in
    assert count[0] == 0


def test_nothing_leaks_between_the_images_of_a_batch():
    a, c = random_map(45, 77, 0.45, 1), serpentine(45, 77)
    table, count, ids = check(np.stack([a, np.zeros_like(a), c]))
    assert count[1] == 0 and (ids[1] == -1).all() and count[2] == 1
    alone = cr.label_components(c, (1,))
    assert np.array_equal(table[2], alone[0][0]) and np.array_equal(ids[2], alone[2][0])


def test_512_square_random_and_blobs():
    blobs = np.zeros((512, 512), np.uint8)
    yy, xx = np.mgrid[:512, :512]
    for cy, cx, r in ((150, 130, 70), (160, 380, 55), (400, 250, 90), (30, 30, 5)):
        blobs[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    table, count, _ = check(np.stack([blobs, random_map(512, 512, 0.5, 3)]), min_area=256, max_out=16)
    assert count[0] == 3


def test_1024_square():
    check(random_map(1024, 1024, 0.45, 9), max_out=64)


def test_python_entry_point():
    m = np.stack([random_map(53, 37, 0.4, 2), checkerboard(53, 37)])
    lab = torch.from_numpy(m).to(DEV)
    table, count, ids = components.label_components(lab, (1,), min_area=2, max_out=5, want_ids=True)
    want = cr.label_components(m, (1,), 2, 5)
    assert table.dtype == torch.int32 and tuple(table.shape) == (2, 5, 6) and tuple(count.shape) == (2,) and tuple(ids.shape) == (2, 53, 37)
    assert np.array_equal(table.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1]) and np.array_equal(ids.cpu().numpy(), want[2])
    t1, c1, none = components.label_components(lab[1], (1,))                     # [H,W]; no ids asked for
    assert none is None and tuple(t1.shape) == (1, 16, 6) and c1.tolist() == [1]
