#!/usr/bin/env python
"""The three owner calls.  mkd_owner_map (two launches) at 512^2 batch 1 / 8 / 16 and 1024^2 batch 1 on three maps: a parser-like map
with a few blobs and some speckle (components from mkd_label_components, min_area (S // 32)^2, max_out 64), 64 single-pixel seeds, and
ONE seed in a corner -- the worst case of the row pass's outward scan: every pixel scans until it reaches the seed's column and on to
the distance found there.  mkd_owner_weights (one launch) at 512^2, 8 planes, feather 0 / 2 / 16.  mkd_paste_photo_weighted against
mkd_paste_photo at tools/bench_photo.py's shape (batch 8, a 2000^2 box of a 4000 x 3000 photo, S 256) with a 512^2 weight plane.
A device sample is the time between two events around --iters back-to-back calls (buffers allocated once, outside), divided by
--iters, median (minimum) over --rounds rounds.  The forms of a comparison are alternated inside the rounds: the owner map with what it
replaces -- the download of ids and table plus one scipy.ndimage.distance_transform_edt per rank on the host (wall clock, up to
seconds a round: three rounds at batch 1, one otherwise, the number is printed; skipped when scipy is not importable) -- and the
weighted paste with the plain one, every round.  The device's owner map is compared with the host's once per case."""
import argparse, ctypes as C, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import components, lib as mlib, photo

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_owner.py measures on the GPU: there is none')
try:
    from scipy import ndimage
except ImportError:
    ndimage = None

lines = []
P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
lib = mlib.load()


def say(text):
    print(text, flush=True)
    lines.append(text)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        call()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


def report(samples):
    return f'{statistics.median(samples):8.4f} ms ({min(samples):.4f})'


def blobs_labels(S, seed):
    """a few filled ellipses (faces) and some speckle, as a parser's label map has them (tools/bench_components.py)"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:S, :S]
    m = np.zeros((S, S), np.uint8)
    for _ in range(4):
        cy, cx, ry, rx = g.uniform(0.15, 0.85) * S, g.uniform(0.15, 0.85) * S, g.uniform(0.06, 0.16) * S, g.uniform(0.05, 0.12) * S
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    m[g.random((S, S)) < 0.002] = 1
    return m


def from_labels(S, B):
    lab = torch.from_numpy(np.stack([blobs_labels(S, 10 * b + S) for b in range(B)])).cuda()
    table, _, ids = components.label_components(lab, (1,), min_area=(S // 32) ** 2, max_out=components.MAX_OUT, want_ids=True)
    return ids, table


def from_seeds(S, B, seeds_of):
    ids = np.full((B, S, S), -1, np.int32)
    table = np.tile(np.array(components.FILL_ROW, np.int32), (B, components.MAX_OUT, 1))
    for b in range(B):
        px = sorted(seeds_of(b))
        ids[b].reshape(-1)[px] = px
        table[b, :len(px), 0] = px
    return torch.from_numpy(ids).cuda(), torch.from_numpy(table).cuda()


INPUTS = (('blobs', from_labels),
          ('64 seeds', lambda S, B: from_seeds(S, B, lambda b: np.random.default_rng(S + b).permutation(S * S)[:64].tolist())),
          ('corner seed', lambda S, B: from_seeds(S, B, lambda b: [0])))


def host_owner(ids, table):
    """what the device call replaces: download, one exact distance transform per rank, the lowest rank on equality"""
    ids, table = ids.cpu().numpy(), table.cpu().numpy()
    out = np.full(ids.shape, components.NO_OWNER, np.uint8)
    for b in range(ids.shape[0]):
        best = np.full(ids.shape[1:], np.inf)
        for r, cid in enumerate(table[b, :, 0].tolist()):
            if cid < 0:
                continue
            d = ndimage.distance_transform_edt(ids[b] != cid)
            d = np.rint(d * d)
            closer = d < best
            out[b][closer], best[closer] = r, d[closer]
    return out


say(f'mkd_owner_map (2 launches), max_out {components.MAX_OUT}, dist2_out written: ms per call = device time between events around '
    f'{args.iters} back-to-back calls / {args.iters}; host form: download + scipy.ndimage.distance_transform_edt per rank, wall clock; '
    f'device median (min) over {args.rounds} rounds, the host form alternated with them for its rounds')
for S, B in ((512, 1), (512, 8), (512, 16), (1024, 1)):
    for name, make in INPUTS:
        ids, table = make(S, B)
        owner = torch.empty((B, S, S), device='cuda', dtype=torch.uint8)
        dist = torch.empty((B, S, S), device='cuda', dtype=torch.int32)
        nbytes = int(lib.mkd_owner_map_scratch_bytes(B, S, S))
        scratch = torch.empty((nbytes + 256,), device='cuda', dtype=torch.uint8)
        base = (scratch.data_ptr() + 255) & ~255

        def device_call():
            mlib.check(lib.mkd_owner_map(P(ids), P(table), B, S, S, components.MAX_OUT, P(owner), P(dist), C.c_void_p(base), stream()), 'mkd_owner_map')

        def timed_host():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_owner(ids, table)
            return (time.perf_counter() - t0) * 1e3

        device_call(); device_call()
        torch.cuda.synchronize()
        dev, hst = [], []
        if ndimage is not None:          # (the comparison is the first host sample; a host round takes up to seconds: 3 at batch 1, else this one)
            t0 = time.perf_counter()
            want = host_owner(ids, table)
            hst.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(owner.cpu().numpy(), want), (name, S, B, int((owner.cpu().numpy() != want).sum()))
        for _ in range(args.rounds):
            dev.append(timed(device_call))
            if ndimage is not None and B == 1 and len(hst) < 3:
                hst.append(timed_host())
        ranks = int((table[:, :, 0] >= 0).sum().item())
        tail = f'   scipy on the host {statistics.median(hst):10.3f} ms ({min(hst):.3f}, {len(hst)} rounds)' if hst else '   scipy on the host: not importable, skipped'
        say(f'    {S}^2 batch {B:2d}  {name:12s} {ranks:5d} ranks  device {report(dev)}{tail}')

say(f'mkd_owner_weights (1 launch), 512^2, owner map of the blobs case at batch 8, 8 planes (image b, rank 0): ms per call as above')
ids, table = from_labels(512, 8)
owner = components.owner_map(ids, table)
items = (C.c_int32 * 16)(*[v for b in range(8) for v in (b, 0)])
w = torch.empty((8, 512, 512), device='cuda', dtype=torch.float32)
for rho in (0, 2, 16):
    call = lambda: mlib.check(lib.mkd_owner_weights(P(owner), 8, 512, 512, items, 8, rho, P(w), stream()), 'mkd_owner_weights')
    call(); call()
    torch.cuda.synchronize()
    say(f'    feather {rho:2d}  device {report([timed(call) for _ in range(args.rounds)])}')

Bp, (Hp, Wp), box, Sp, rho = 8, (3000, 4000), (1000, 500, 2000, 2000), 256, 8
say(f'mkd_paste_photo_weighted against mkd_paste_photo: batch {Bp}, box {box[2]} x {box[3]} of a {Wp} x {Hp} photo, S {Sp}, feather {rho}, weights '
    f'{Bp} x 512^2 in [0, 1]: ms per call as above, the two forms alternated within each round')
g = torch.Generator().manual_seed(5)
work = list(torch.randint(0, 256, (Bp, Hp, Wp, 3), generator=g, dtype=torch.uint8).cuda().unbind(0))
s01 = torch.rand((Bp, 3, Sp, Sp), generator=g).cuda()
t = (torch.rand((Bp, 3, Sp, Sp), generator=g) * 2.0 - 1.0).cuda()
wts = torch.rand((Bp, 512, 512), generator=g).cuda()
boxes = [box] * Bp
forms = {'mkd_paste_photo': lambda: photo.paste_photos(work, boxes, t, s01, rho),
         'mkd_paste_photo_weighted': lambda: photo.paste_photos(work, boxes, t, s01, rho, weights=wts)}
for f in forms.values():
    f(); f()
torch.cuda.synchronize()
samples = {k: [] for k in forms}
for _ in range(args.rounds):
    for k, f in forms.items():
        samples[k].append(timed(f))
for k, v in samples.items():
    say(f'    {k:26s} device {report(v)}')
say(f'    weighted / plain (medians): {statistics.median(samples["mkd_paste_photo_weighted"]) / statistics.median(samples["mkd_paste_photo"]):.3f}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
