#!/usr/bin/env python
"""mkd_label_components (connected components of a label map, four launches) at 512^2 batch 1 / 8 / 16 and 1024^2 batch 1, on three
inputs: a parser-like map with a few blobs, a 50 %-density random map and ONE serpentine component (a line one pixel wide through
every tile: the worst case of the seam merge).  A device sample is the time between two events around --iters back-to-back calls
(the scratch allocated once, outside), divided by --iters; each is alternated, inside every round, with what the call replaces:
the download of the label maps plus scipy.ndimage.label + find_objects on the host (wall clock; skipped when scipy is not
importable).  Median (minimum) over --rounds rounds.  The device result is compared with scipy's once per case."""
import argparse, ctypes as C, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import components, lib as mlib

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--max-out', type=int, default=16)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_components.py measures on the GPU: there is none')
try:
    from scipy import ndimage
except ImportError:
    ndimage = None

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def blobs_map(S, seed):
    """a few filled ellipses (faces) and some speckle, as a parser's label map has them"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:S, :S]
    m = np.zeros((S, S), np.uint8)
    for _ in range(4):
        cy, cx, ry, rx = g.uniform(0.15, 0.85) * S, g.uniform(0.15, 0.85) * S, g.uniform(0.06, 0.16) * S, g.uniform(0.05, 0.12) * S
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    m[g.random((S, S)) < 0.002] = 1
    return m


def random_map(S, seed):
    return (np.random.default_rng(seed).random((S, S)) < 0.5).astype(np.uint8)


def serpentine(S, seed):
    m = np.zeros((S, S), np.uint8)
    m[::2] = 1
    for k, y in enumerate(range(1, S - 1, 2)):
        m[y, S - 1 if k % 2 == 0 else 0] = 1
    return m


INPUTS = (('blobs', blobs_map), ('random 50 %', random_map), ('serpentine', serpentine))
lib = mlib.load()
say(f'mkd_label_components, classes (1,), min_area 1, max_out {args.max_out}, ids_out written: ms per call = device time between events around '
    f'{args.iters} back-to-back calls / {args.iters}; host form: download + scipy.ndimage.label (8-connected) + find_objects per image, wall '
    f'clock; median (min) over {args.rounds} rounds, forms alternated within each round')
for S, B in ((512, 1), (512, 8), (512, 16), (1024, 1)):
    for name, make in INPUTS:
        host = np.stack([make(S, 10 * b + S) for b in range(B)])
        lab = torch.from_numpy(host).cuda()
        table = torch.empty((B, args.max_out, 6), device='cuda', dtype=torch.int32)
        count = torch.empty((B,), device='cuda', dtype=torch.int32)
        ids = torch.empty((B, S, S), device='cuda', dtype=torch.int32)
        nbytes = int(lib.mkd_label_components_scratch_bytes(B, S, S))
        scratch = torch.empty((nbytes + 256,), device='cuda', dtype=torch.uint8)
        base = (scratch.data_ptr() + 255) & ~255
        P = lambda t: C.c_void_p(t.data_ptr())

        def device_call():
            mlib.check(lib.mkd_label_components(P(lab), B, S, S, C.c_uint64(2), 1, args.max_out, P(table), P(count), P(ids), C.c_void_p(base),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mkd_label_components')

        def host_call():
            out = []
            for m in lab.cpu().numpy():
                l, n = ndimage.label(m == 1, structure=np.ones((3, 3)))
                out.append((n, ndimage.find_objects(l)))
            return out

        def timed():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                device_call()
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) / args.iters

        def timed_host():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_call()
            return (time.perf_counter() - t0) * 1e3

        device_call(); device_call()
        torch.cuda.synchronize()
        if ndimage is not None:
            got = count.cpu().tolist()
            want = [n for n, _ in host_call()]
            assert got == want, (name, S, B, got, want)
        dev, hst = [], []
        for _ in range(args.rounds):
            dev.append(timed())
            if ndimage is not None:
                hst.append(timed_host())
        comps = int(count.sum().item())
        tail = f'   scipy on the host {statistics.median(hst):9.3f} ms ({min(hst):.3f})' if hst else '   scipy on the host: not importable, skipped'
        say(f'    {S}^2 batch {B:2d}  {name:12s} {comps:7d} components  device {statistics.median(dev):8.4f} ms ({min(dev):.4f}){tail}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
