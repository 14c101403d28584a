#!/usr/bin/env python
"""What the noise of one sampling call costs, three ways, at the flagship shape: 50 rows of a batch of 8 latents of 4 x 32 x 32
([50][8 * 4 * 32 * 32] fp32, 1.6 M values).
  mkd_noise_fill      the counter-based generator, ONE launch for the whole tensor (double log / sqrt / sincospi per pair of values)
  torch.randn         the same shape on the device generator (one launch)
  host draw of x_T    what runs/test.py --seed does per batch of 8 today: one torch.Generator per pair, a host randn of [1,4,32,32]
                      each, a cat and the copy to the device (x_T only: 8 * 4096 values; host clock around a synchronise)
A device sample is the time between two events around --iters back-to-back calls (buffers allocated once, outside), divided by --iters,
median (minimum) over --rounds rounds; the two device forms are alternated inside the rounds."""
import argparse, ctypes as C, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import lib as mlib

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--rows', type=int, default=50)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--latent', type=int, default=32)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_noise.py measures on the GPU: there is none')

lines = []
R, B, h = args.rows, args.batch, args.latent
n = 4 * h * h


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        call()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


lib = mlib.load()
seeds = torch.arange(B, dtype=torch.int64, device='cuda')
out = torch.empty(R, B, n, dtype=torch.float32, device='cuda')
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fill():
    rc = lib.mkd_noise_fill(C.c_void_p(seeds.data_ptr()), None, B, 1, 0, R, n, 0, C.c_void_p(out.data_ptr()), stream)
    assert rc == 0, lib.mkd_last_error()


def randn():
    torch.randn(out.shape, device='cuda', out=out)


def host_x_T():
    x = torch.cat([torch.randn(1, 4, h, h, generator=torch.Generator().manual_seed(3 + i)) for i in range(B)]).cuda()
    torch.cuda.synchronize()
    return x


forms = {'mkd_noise_fill  (1 launch, double Box-Muller)': fill, 'torch.randn on the device (same shape)': randn}
for f in forms.values():
    f(); f()
host_x_T()
torch.cuda.synchronize()
say(f'noise of one sampling call: [{R}][{B} * 4 * {h} * {h}] fp32 = {R * B * n / 1e6:.2f} M values, {R * B * n * 4 / 1e6:.1f} MB written')
say(f'us per call = device time between events around {args.iters} back-to-back calls / {args.iters}; median (min) over {args.rounds} rounds, forms alternated')
samples = {k: [] for k in forms}
for _ in range(args.rounds):
    for k, f in forms.items():
        samples[k].append(timed(f))
for k, v in samples.items():
    med = statistics.median(v)
    say(f'    {k:48s} device {med * 1e3:10.1f} us ({min(v) * 1e3:.1f})   {R * B * n / med / 1e6:8.2f} G values/s')
host = []
for _ in range(args.rounds * 4):
    t0 = time.perf_counter()
    host_x_T()
    host.append((time.perf_counter() - t0) * 1e3)
say(f'    {"host draw of x_T alone (runs/test.py --seed, batch " + str(B) + ")":48s} host   {statistics.median(host) * 1e3:10.1f} us ({min(host) * 1e3:.1f})   '
    f'{B * n / 1e3:.1f} K values: per pair a Generator, a randn, then cat and the copy to the device')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
