"""-m gpu: mkd_owner_map and mkd_owner_weights against the numpy restatement (tests/owner_ref.py), exactly: owner and dist2 bytes
against brute force over all seeds, the weights' bits against numpy's.  Every owner-map case runs twice, into differently poisoned
outputs and scratch, and the two runs must give the same bytes.  The shapes sit where the kernels can go wrong (one pixel, one row, one
column, more than one wave of columns, the x loop beyond one workgroup, the longest side with the longest scan), not at the
workload's size."""
import ctypes as C

import numpy as np
import pytest
import torch

import owner_ref as orf
from makeupdiffuse_amd import components
from makeupdiffuse_amd import lib as mlib

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FILL = -1


def P(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def make_table(rows_per_image, max_out):
    """lists of component ids -> int32 [B, max_out, 6]; only the id column is read, the others are poisoned"""
    t = np.full((len(rows_per_image), max_out, 6), 0x5A5A5A5A, np.int32)
    t[:, :, 0] = FILL
    for b, rows in enumerate(rows_per_image):
        t[b, :len(rows), 0] = rows
    return t


def device_run(ids: np.ndarray, table: np.ndarray, poison, want_dist=True):
    """one library call with the outputs and the scratch filled with ``poison`` bytes first -> (owner, dist2) as numpy"""
    lib = mlib.load()
    B, H, W = ids.shape
    d_ids, d_table = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
    owner = torch.full((B, H, W), poison, device=DEV, dtype=torch.uint8)
    dist = torch.full((B, H, W * 4), poison, device=DEV, dtype=torch.uint8) if want_dist else None
    nbytes = int(lib.mkd_owner_map_scratch_bytes(B, H, W))
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.full((nbytes + 256,), poison, device=DEV, dtype=torch.uint8)
    base = (scratch.data_ptr() + 255) & ~255
    rc = lib.mkd_owner_map(P(d_ids), P(d_table), B, H, W, int(table.shape[1]), P(owner), P(dist), C.c_void_p(base),
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mkd_last_error()
    torch.cuda.synchronize()
    return owner.cpu().numpy(), None if dist is None else dist.cpu().numpy().view(np.int32).reshape(B, H, W)


def check(ids, rows_per_image, max_out=None):
    ids = np.asarray(ids, np.int32)
    if ids.ndim == 2:
        ids, rows_per_image = ids[None], [rows_per_image]
    table = make_table(rows_per_image, max_out or max(1, max(len(r) for r in rows_per_image)))
    want = [orf.owner_brute(i, t[:, 0].tolist()) for i, t in zip(ids, table)]
    want_o, want_d = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    one, two = device_run(ids, table, 0xCD), device_run(ids, table, 0x3B)
    for name, w, a, b in zip(('owner', 'dist2'), (want_o, want_d), one, two):
        assert a.tobytes() == b.tobytes(), f'{name}: two runs differ'
        assert np.array_equal(a, w), f'{name}: {int((a != w).sum())} of {a.size} entries differ from brute force'
    only_owner, none = device_run(ids, table, 0x77, want_dist=False)          # dist2_out NULL
    assert none is None and np.array_equal(only_owner, want_o)
    return want_o, want_d


def blob_ids(H, W, boxes):
    """filled rectangles (r0, r1, c0, c1), clipped to the map -> (ids, their component ids)"""
    return orf.ids_of_seeds(H, W, [[(y, x) for y in range(max(r0, 0), min(r1, H - 1) + 1) for x in range(max(c0, 0), min(c1, W - 1) + 1)]
                                   for r0, r1, c0, c1 in boxes])


def test_one_pixel():
    o, d = check(np.zeros((1, 1)), [0])
    assert o.item() == 0 and d.item() == 0
    o, d = check(np.full((1, 1), -1), [])
    assert o.item() == orf.NO_OWNER and d.item() == orf.NO_DIST


@pytest.mark.parametrize('H,W', [(1, 37), (37, 1)])
def test_one_row_one_column(H, W):
    n = H * W
    ids, comps = orf.ids_of_seeds(H, W, [divmod(k, W) for k in (3, 20, 30)])
    o, d = check(ids, [comps[1], comps[2], comps[0]])
    assert d.reshape(n)[0] == 9 and o.reshape(n)[0] == 2 and o.reshape(n)[36] == 1


@pytest.mark.parametrize('H,W', [(33, 65), (65, 33)])
def test_three_blobs(H, W):
    ids, comps = blob_ids(H, W, [(2, 9, 3, 12), (H - 12, H - 3, W - 20, W - 4), (H // 2 - 2, H // 2 + 2, 0, 4)])
    o, d = check(ids, comps)
    assert set(np.unique(o)) == {0, 1, 2}


def test_64_single_pixel_seeds_use_every_rank():
    px = np.random.default_rng(64).permutation(64 * 64)[:64]
    ids, comps = orf.ids_of_seeds(64, 64, [divmod(int(p), 64) for p in px])
    o, d = check(ids, comps, max_out=64)
    assert set(np.unique(o)) == set(range(64))


def test_the_x_loop_beyond_one_workgroup():
    H, W = 70, 300
    ids, comps = blob_ids(H, W, [(5, 20, 10, 40), (40, 60, 270, 299), (30, 34, 230, 238)])
    ids[0, 299] = 299                                   # one more component, not in the table
    o, d = check(ids, comps)
    assert (o[0, :, 256:] == 1).any() and (o[0, :, 256:] == 2).any() and o[0, 0, 299] != orf.NO_OWNER and d[0, 0, 299] > 0


@pytest.mark.parametrize('H,W,corner', [(2048, 3, (0, 0)), (3, 2048, (2, 2047)), (2048, 3, (2047, 2)), (3, 2048, (0, 0))])
def test_the_longest_side_with_one_corner_seed(H, W, corner):
    ids, comps = orf.ids_of_seeds(H, W, [corner])
    o, d = check(ids, comps)
    assert (o == 0).all() and d.max() == 2047 ** 2 + 2 ** 2


def test_a_batch_with_different_tables_and_an_empty_one():
    H, W = 20, 45
    a, ca = blob_ids(H, W, [(1, 5, 1, 8), (12, 18, 30, 44)])
    b, cb = blob_ids(H, W, [(8, 11, 20, 25)])                     # its component is NOT in its (all-empty) table
    c, cc = blob_ids(H, W, [(0, 3, 40, 44), (15, 19, 0, 5), (9, 10, 22, 23)])
    o, d = check(np.stack([a, b, c]), [ca[::-1], [], cc], max_out=5)
    assert (o[1] == orf.NO_OWNER).all() and (d[1] == orf.NO_DIST).all()
    assert o[0, 2, 2] == 1 and o[0, 15, 40] == 0 and set(np.unique(o[2])) == {0, 1, 2}


@pytest.mark.parametrize('name,ids,table', orf.tie_layouts(), ids=[t[0] for t in orf.tie_layouts()])
def test_ties_go_to_the_lower_rank(name, ids, table):
    o, d = check(ids, table)
    H, W = ids.shape
    (ya, xa), (yb, xb) = (divmod(t, W) for t in table)
    yy, xx = np.mgrid[:H, :W]
    tied = (yy - ya) ** 2 + (xx - xa) ** 2 == (yy - yb) ** 2 + (xx - xb) ** 2
    assert tied.sum() >= 3 and (o[0][tied] == 0).all()


def test_only_table_components_are_seeds_and_a_repeated_id_counts_once():
    ids, comps = blob_ids(12, 40, [(0, 2, 0, 2), (5, 6, 18, 20), (9, 11, 36, 39)])
    o, d = check(ids, [comps[0], comps[2]])                       # the middle blob is in no table row
    assert set(np.unique(o)) == {0, 1} and d[0, 5, 19] > 0
    o, d = check(ids, [comps[2], FILL, comps[0], comps[2], comps[0]])          # fill row in between; repeats: the lowest row wins
    assert set(np.unique(o)) == {0, 2} and o[0, 10, 38] == 0 and o[0, 1, 1] == 2


def test_label_components_then_owner_map():
    g = np.random.default_rng(7)
    lab = np.zeros((2, 50, 70), np.uint8)
    lab[0, 5:20, 5:25] = 1; lab[0, 30:45, 40:66] = 1; lab[0, 25, 2] = 1; lab[1, 10:40, 20:30] = 1
    lab[1][g.random((50, 70)) < 0.01] = 1                          # speckle below min_area, some of it touching the blob
    d_lab = torch.from_numpy(lab).to(DEV)
    table, count, ids = components.label_components(d_lab, (1,), min_area=9, max_out=4, want_ids=True)
    owner, dist = components.owner_map(ids, table, want_dist=True)
    assert owner.dtype == torch.uint8 and dist.dtype == torch.int32 and tuple(owner.shape) == tuple(dist.shape) == (2, 50, 70)
    table, ids, owner, dist = table.cpu().numpy(), ids.cpu().numpy(), owner.cpu().numpy(), dist.cpu().numpy()
    assert count.cpu().tolist() == [2, 1]
    for b in range(2):
        for r in range(4):
            if table[b, r, 0] >= 0:
                at = ids[b] == table[b, r, 0]
                assert at.sum() == table[b, r, 1] and (owner[b][at] == r).all() and (dist[b][at] == 0).all()
        wo, wd = orf.owner_brute(ids[b], table[b, :, 0].tolist())
        assert np.array_equal(owner[b], wo) and np.array_equal(dist[b], wd)
    assert dist[0, 25, 2] > 0                                      # the single pixel is below min_area: owned, not a seed
    assert torch.equal(components.owner_map(torch.from_numpy(ids).to(DEV), torch.from_numpy(table).to(DEV)).cpu(), torch.from_numpy(owner))


# ---- weights ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def owner_maps():
    g = np.random.default_rng(40)
    o = np.zeros((2, 40, 56), np.uint8)
    o[0, :, 30:] = 1; o[0, 25:, :20] = 2; o[0, 0, 0] = 1; o[0, 39, 55] = 0          # regions, and corners that differ from their surroundings
    o[1] = g.integers(0, 4, (40, 56))
    o[1, :3, :3] = 63
    return o


@pytest.mark.parametrize('rho', [0, 1, 16])
def test_weights_have_numpys_bits(owner_maps, rho):
    items = [(0, 0), (0, 1), (1, 3), (0, 2), (1, 63), (1, 7)]          # (the last owns nothing: all zero)
    got = components.owner_weights(torch.from_numpy(owner_maps).to(DEV), items, rho).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(items), 40, 56)
    for k, (b, r) in enumerate(items):
        want = orf.weights(owner_maps[b], r, rho)
        assert got[k].tobytes() == want.tobytes(), f'item {(b, r)}: {int((got[k] != want).sum())} weights differ'
    assert (got[5] == 0).all()
    if rho == 0:
        assert set(np.unique(got)) == {0.0, 1.0}
    total = sum(orf.weights(owner_maps[0], r, rho).astype(np.float64) for r in range(3))
    assert np.abs(total - 1.0).max() < 1e-6                       # a partition: the faces' shares of a neighbourhood sum to one


def test_more_items_than_one_call_takes(owner_maps):
    items = [(k % 2, k % 4) for k in range(19)]
    got = components.owner_weights(torch.from_numpy(owner_maps).to(DEV), items, 2).cpu().numpy()
    for k, (b, r) in enumerate(items):
        assert got[k].tobytes() == orf.weights(owner_maps[b], r, 2).tobytes()


# ---- errors leave the outputs alone ------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    lib = mlib.load()
    B, H, W = 2, 9, 11
    ids = torch.full((B, H, W), -1, device=DEV, dtype=torch.int32)
    table = torch.from_numpy(make_table([[], []], 4)).to(DEV)
    owner = torch.full((B, H, W), 0xA7, device=DEV, dtype=torch.uint8)
    dist = torch.full((B, H, W * 4), 0xA7, device=DEV, dtype=torch.uint8)
    scratch = torch.empty((int(lib.mkd_owner_map_scratch_bytes(B, H, W)) + 512,), device=DEV, dtype=torch.uint8)
    base = (scratch.data_ptr() + 255) & ~255
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(ids=P(ids), table=P(table), batch=B, H=H, W=W, max_out=4, owner=P(owner), dist=P(dist), scratch=C.c_void_p(base))
    for bad in (dict(batch=0), dict(batch=65536), dict(H=0), dict(W=2049), dict(H=2049), dict(max_out=0), dict(max_out=65), dict(ids=None),
                dict(table=None), dict(scratch=None), dict(scratch=C.c_void_p(base + 16))):
        a = dict(good, **bad)
        rc = lib.mkd_owner_map(a['ids'], a['table'], a['batch'], a['H'], a['W'], a['max_out'], a['owner'], a['dist'], a['scratch'], st)
        assert rc == -1 and lib.mkd_last_error(), bad
    w = torch.full((2, H, W * 4), 0xA7, device=DEV, dtype=torch.uint8)
    for items, n, rho in (([(2, 0)], 1, 2), ([(0, 64)], 1, 2), ([(-1, 0)], 1, 2), ([(0, -1)], 1, 2), ([(0, 0)], 0, 2), ([(0, 0)] * 17, 17, 2),
                          ([(0, 0)], 1, 17), ([(0, 0)], 1, -1)):
        flat = (C.c_int32 * (2 * len(items)))(*[v for it in items for v in it])
        assert lib.mkd_owner_weights(P(owner), B, H, W, flat, n, rho, P(w), st) == -1 and lib.mkd_last_error(), (items, n, rho)
    torch.cuda.synchronize()
    assert (owner == 0xA7).all() and (dist == 0xA7).all() and (w == 0xA7).all()
