"""CPU: the restatement of mkd_owner_map (tests/owner_ref.py) -- brute force over all seeds against one scipy distance transform per
rank, ties included --, find_faces(return_owner=True) with its device calls stubbed, the library's argument checks of the three new
entries (they run before anything is enqueued, so they need no device), transfer_photos(own_pixels=...)'s own checks and the flags of
runs/test.py."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import components_ref as cr
import owner_ref as orf
from makeupdiffuse_amd import components
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import lib as mlib
from test_components_host import StubParser, _model, host_components, stub_resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------
def random_case(k):
    """sizes 1..20 per side, 0..6 ranks; a component is 1..4 pixels anywhere (the owner map asks nothing of their shape), some ids
    stay out of the table, some table rows are fill rows"""
    g = np.random.default_rng(500 + k)
    H, W = int(g.integers(1, 21)), int(g.integers(1, 21))
    n_rank = int(g.integers(0, 7))
    ids = np.full((H, W), -1, np.int32)
    free = g.permutation(H * W).tolist()
    comps = []
    for _ in range(n_rank + int(g.integers(0, 3))):                   # the extra ones are not in the table: not seeds
        px = [free.pop() for _ in range(min(len(free), int(g.integers(1, 5))))]
        if not px:
            break
        ids.reshape(-1)[px] = min(px)
        comps.append(min(px))
    table = comps[:n_rank] + [-1] * int(g.integers(0, 3))
    return ids, table


@pytest.mark.parametrize('k', range(40))
def test_brute_force_agrees_with_scipy_per_rank(k):
    pytest.importorskip('scipy.ndimage')
    ids, table = random_case(k)
    o1, d1 = orf.owner_brute(ids, table)
    o2, d2 = orf.owner_edt(ids, table)
    assert np.array_equal(o1, o2) and np.array_equal(d1, d2)
    if not any(t >= 0 for t in table):
        assert (o1 == orf.NO_OWNER).all() and (d1 == orf.NO_DIST).all()
    else:
        rank = orf.seed_ranks(ids, table)
        assert np.array_equal(o1[rank >= 0], rank[rank >= 0]) and (d1[rank >= 0] == 0).all() and (d1[rank < 0] > 0).all()


@pytest.mark.parametrize('name,ids,table', orf.tie_layouts(), ids=[t[0] for t in orf.tie_layouts()])
def test_ties_go_to_the_lower_rank(name, ids, table):
    pytest.importorskip('scipy.ndimage')
    o1, d1 = orf.owner_brute(ids, table)
    o2, d2 = orf.owner_edt(ids, table)
    assert np.array_equal(o1, o2) and np.array_equal(d1, d2)
    H, W = ids.shape
    (ya, xa), (yb, xb) = (divmod(t, W) for t in table)
    yy, xx = np.mgrid[:H, :W]
    tied = (yy - ya) ** 2 + (xx - xa) ** 2 == (yy - yb) ** 2 + (xx - xb) ** 2
    assert tied.sum() >= 3 and (o1[tied] == 0).all()                  # whichever of the two components is rank 0


def test_a_repeated_id_counts_for_its_lowest_row_and_weights_are_window_fractions():
    ids, (a, b) = orf.ids_of_seeds(4, 6, [(0, 0), (3, 5)])
    assert orf.seed_ranks(ids, [a, b, a, -1])[0, 0] == 0 and orf.seed_ranks(ids, [b, a, a])[0, 0] == 1
    owner = np.array([[0, 0, 1], [0, 1, 1], [255, 1, 1]], np.uint8)
    assert np.array_equal(orf.weights(owner, 1, 0), (owner == 1).astype(np.float32))
    w = orf.weights(owner, 0, 1)
    assert w.dtype == np.float32 and w[1, 1] == np.float32(3) / np.float32(9)
    assert w[0, 0] == np.float32(8) / np.float32(9)                   # the clamped corner: (0, 0) four times, (0, 1) and (1, 0) twice, (1, 1) once
    assert np.array_equal(orf.weight_at_photo(np.ones((3, 5), np.float32), 7, 11), np.ones((7, 11), np.float32))


# ---- find_faces(return_owner=True): both device calls stubbed ----------------------------------------------------------------------
def host_components_with_ids(seen):
    def components_of(labels, classes, min_area=1, max_out=16, want_ids=False):
        seen.append((min_area, max_out, want_ids))
        t, c, ids = cr.label_components(labels.numpy(), classes, min_area, max_out)
        return torch.from_numpy(t), torch.from_numpy(c), torch.from_numpy(ids.astype(np.int32))
    return components_of


def test_find_faces_return_owner_keeps_the_boxes_and_seeds_every_row():
    S = 64
    maps = torch.zeros(2, S, S, dtype=torch.uint8)
    blobs = [(30, 49, 5, 20), (2, 9, 40, 47), (52, 60, 50, 61), (20, 21, 60, 61)]          # areas 320, 64, 108, 4
    for r0, r1, c0, c1 in blobs:
        maps[0, r0:r1 + 1, c0:c1 + 1] = 1
    maps[0, 0, 0] = 1                                                                    # speckle below min_area = 4: never a seed
    photos = [torch.zeros(300, 200, 3, dtype=torch.uint8), torch.zeros(90, 120, 3, dtype=torch.uint8)]
    seen, tables = [], []

    def owner_of(ids, table):
        tables.append(table.clone())
        out = [orf.owner_brute(i, t[:, 0].tolist())[0] for i, t in zip(ids.numpy(), table.numpy())]
        return torch.from_numpy(np.stack(out))

    plain = fp.find_faces(StubParser(maps), photos, max_faces=2, parse_size=S, resize=stub_resize, components_of=host_components())
    faces, owner = fp.find_faces(StubParser(maps), photos, max_faces=2, parse_size=S, resize=stub_resize,
                                 components_of=host_components_with_ids(seen), return_owner=True, owner_of=owner_of)
    assert faces == plain and [len(f) for f in faces] == [2, 0]                          # the same rows, the same boxes
    assert seen == [((S // 32) ** 2, components.MAX_OUT, True)]
    assert tuple(tables[0].shape) == (2, components.MAX_OUT, 6) and (tables[0][0, :, 0] >= 0).sum() == 4          # ALL four rows are seeds
    assert owner.dtype == torch.uint8 and tuple(owner.shape) == (2, S, S)
    o = owner.numpy()
    assert (o[1] == orf.NO_OWNER).all()                                                  # the faceless photo
    for rank, (r0, r1, c0, c1) in enumerate([blobs[0], blobs[2], blobs[1], blobs[3]]):  # by area; ranks 2 and 3 lie beyond max_faces
        assert (o[0, r0:r1 + 1, c0:c1 + 1] == rank).all()
    assert o[0, 0, 0] == 0                                                               # the speckle pixel belongs to its nearest FACE: 925 < 1604


# ---- the library's argument checks: before anything is enqueued, so they run without a device --------------------------------------
MAP_GOOD = dict(ids=0x1000, table=0x2000, batch=2, H=40, W=50, max_out=16, owner=0x3000, dist=None, scratch=0x4000)
MAP_BAD = [dict(batch=0), dict(batch=65536), dict(H=0), dict(W=0), dict(H=2049), dict(W=2049), dict(max_out=0), dict(max_out=65), dict(ids=None),
           dict(table=None), dict(owner=None), dict(scratch=None), dict(scratch=0x4010)]


@pytest.mark.parametrize('bad', MAP_BAD, ids=[str(b) for b in MAP_BAD])
def test_owner_map_refuses_bad_arguments(bad):
    lib = mlib.load()
    a = dict(MAP_GOOD, **bad)
    rc = lib.mkd_owner_map(C.c_void_p(a['ids']), C.c_void_p(a['table']), a['batch'], a['H'], a['W'], a['max_out'], C.c_void_p(a['owner']),
                           C.c_void_p(a['dist']), C.c_void_p(a['scratch']), None)
    assert rc == -1 and lib.mkd_last_error()          # MKD_ERR_ARG


def test_owner_map_scratch_bytes():
    lib = mlib.load()
    for args in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 2049, 8), (1, 8, 2049)):
        assert lib.mkd_owner_map_scratch_bytes(*args) == 0
    one = lib.mkd_owner_map_scratch_bytes(3, 37, 53)
    assert one % 256 == 0 and 3 * 3 * 37 * 53 <= one < 3 * 3 * 37 * 53 + 512
    assert lib.mkd_owner_map_scratch_bytes(1, 2048, 2048) == 3 * 2048 * 2048


W_GOOD = dict(owner=0x1000, batch=2, H=40, W=50, items=[(0, 0), (1, 63)], n=None, feather=2, out=0x2000)
W_BAD = [dict(items=[(2, 0)]), dict(items=[(-1, 0)]), dict(items=[(0, 64)]), dict(items=[(0, -1)]), dict(n=0), dict(items=[(0, 0)] * 17),
         dict(feather=-1), dict(feather=17), dict(owner=None), dict(out=None), dict(items=None), dict(H=0), dict(W=2049), dict(batch=0)]


@pytest.mark.parametrize('bad', W_BAD, ids=[str(b) for b in W_BAD])
def test_owner_weights_refuses_bad_arguments(bad):
    lib = mlib.load()
    a = dict(W_GOOD, **bad)
    items = a['items']
    flat = None if items is None else (C.c_int32 * (2 * len(items)))(*[v for it in items for v in it])
    n = a['n'] if a['n'] is not None else (1 if items is None else len(items))
    rc = lib.mkd_owner_weights(C.c_void_p(a['owner']), a['batch'], a['H'], a['W'], flat, n, a['feather'], C.c_void_p(a['out']), None)
    assert rc == -1 and lib.mkd_last_error()


def test_paste_photo_weighted_refuses_bad_arguments():
    lib = mlib.load()
    d = (mlib.PhotoDescC * 1)()
    d[0].pixels, d[0].pitch_bytes, d[0].H, d[0].W, d[0].x0, d[0].y0, d[0].bw, d[0].bh = 0x1000, 300, 80, 100, 10, 10, 40, 40
    call = lambda w=0x4000, wh=16, ww=16, t=0x2000, feather=3: lib.mkd_paste_photo_weighted(d, 1, 64, C.c_void_p(t), C.c_void_p(0x3000), feather,
                                                                                         C.c_void_p(w), wh, ww, None)
    for kw in (dict(w=None), dict(ww=2049), dict(wh=2049), dict(ww=0), dict(wh=0), dict(t=None), dict(feather=65)):
        assert call(**kw) == -1 and lib.mkd_last_error(), kw
    d[0].bw = 200                                     # the descriptor checks of mkd_paste_photo hold here too
    assert call() == -1


def test_python_side_checks():
    ids, table = torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 4, 6, dtype=torch.int32)
    with pytest.raises(mlib.MkdError):
        components.owner_map(ids, table)                             # CPU tensors: there is no CPU path
    for bad_ids, bad_table in ((ids.long(), table), (ids[0], table), (ids, table[:, :, :5]), (ids, table.long()), (ids, torch.zeros(2, 4, 6, dtype=torch.int32))):
        with pytest.raises(ValueError):
            components.owner_map(bad_ids, bad_table)
    owner = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError):
        components.owner_weights(owner, [(0, 0)], 2)
    with pytest.raises(ValueError):
        components.owner_weights(owner.int(), [(0, 0)], 2)


# ---- transfer_photos(own_pixels=...): what it checks before it touches the device ---------------------------------------------------
def test_transfer_photos_own_pixels_checks():
    m = _model()
    p = [torch.zeros(80, 80, 3, dtype=torch.uint8)] * 2
    one, ref = (0, 0, 40, 40), [(0, 0, 80, 80)] * 2
    with pytest.raises(ValueError, match='own_pixels'):
        m.transfer_photos(p, p, [[one], []], ref, max_faces=2, own_pixels=True)          # explicit boxes: no component owns anything
    with pytest.raises(ValueError, match='own_pixels'):
        m.transfer_photos(p, p, None, ref, max_faces=2, own_pixels=True)                 # no face parser
    with pytest.raises(ValueError, match='own_pixels only applies with max_faces'):
        m.transfer_photos(p, p, [one, one], ref, own_pixels=True)
    m.face_parser = object()
    for bad in (-1, 17, 1.5):
        with pytest.raises(ValueError, match='own_feather'):
            m.transfer_photos(p, p, None, ref, max_faces=2, own_pixels=True, own_feather=bad)


# ---- runs/test.py ------------------------------------------------------------------------------------------------------------------
def test_runs_test_own_pixels_flags(monkeypatch, tmp_path):
    spec = importlib.util.spec_from_file_location('runs_test_cli_owned', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args([])
    assert args.own_pixels is False and args.own_feather == 2
    args = mod.build_parser().parse_args(['--photos', '--max-faces', '3', '--own-pixels', '--own-feather', '4'])
    assert args.own_pixels is True and args.own_feather == 4

    def refused(*argv):
        monkeypatch.setattr(sys, 'argv', ['test.py', *argv])
        with pytest.raises(SystemExit) as e:
            mod.main()
        return str(e.value)

    root = str(tmp_path)
    assert '--own-pixels only applies with --photos --max-faces' in refused('--own-pixels')
    assert '--own-pixels only applies with --photos --max-faces' in refused('--own-pixels', '--photos', '--data-root', root, '--face-parser', 'random')
    assert '--own-feather only applies with --own-pixels' in refused('--own-feather', '3', '--photos', '--data-root', root, '--max-faces', '2',
                                                                     '--face-parser', 'random')
    assert '--own-feather must be 0..16' in refused('--own-pixels', '--own-feather', '17', '--photos', '--data-root', root, '--max-faces', '2',
                                                   '--face-parser', 'random')
    (tmp_path / 'boxes.txt').write_text('a.png 0 0 8 8\n')                               # faces from a boxes file own nothing
    for parser in ((), ('--face-parser', 'random')):
        assert '--own-pixels needs the faces from --face-parser' in refused('--own-pixels', '--photos', '--data-root', root, '--max-faces', '2', *parser)
