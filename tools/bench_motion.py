#!/usr/bin/env python
"""mkd_motion_warp at the video workload: n = 8 faces of one frame step at S = 256, every face with a previous frame (this frame's
luminance displaced by one pixel, so the search finds a match), search 1, 3 and 7 and both block sizes; one launch each.  Beside it
mkd_temporal_diff (radius 1) on the warped pools, the call it sits in front of.  A device sample is the time between two events around
--iters back-to-back calls (buffers allocated once, outside), divided by --iters, median (minimum) over --rounds rounds; the forms are
alternated inside the rounds.  Bytes per call are counted from the shapes: s01, D_in and Y_in read, D_w and Y_w written, all fp32."""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import video

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=50)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_motion.py measures on the GPU: there is none')

lines = []
B, S = args.batch, args.size


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


g = torch.Generator().manual_seed(31)
byte = torch.randint(0, 256, (B, 3, S, S), generator=g)
s01 = (byte.float() / 255.0).cuda()
t = (torch.rand((B, 3, S, S), generator=g) * 2.0 - 1.0).cuda()
out = torch.empty_like(t)
luma = (77 * byte[:, 0] + 150 * byte[:, 1] + 29 * byte[:, 2]).float()
D_in = (torch.rand((B, 3, S, S), generator=g) - 0.5).cuda()
Y_in = torch.roll(luma, (1, -1), (1, 2)).cuda()
D_w, Y_w = torch.zeros_like(D_in), torch.zeros_like(Y_in)
D_out, Y_out = torch.zeros_like(D_in), torch.zeros_like(Y_in)
slots = list(range(B))
filt = video.TemporalFilter(0.8, 4.0, 1)
forms = {}
for block in (16, 8):
    nb = -(-S // block)
    vec = torch.zeros((B, nb, nb, 2), dtype=torch.int32, device='cuda')
    for search in (1, 3, 7):
        forms[f'mkd_motion_warp  block {block:2d}  search {search} ({(2 * search + 1) ** 2:3d} candidates)'] = (
            lambda ms=video.MotionSearch(search, block, 256), v=vec: video.motion_warp(s01, D_in, Y_in, slots, D_w, Y_w, ms, v))
forms['mkd_temporal_diff  R 1 (the call it feeds)'] = lambda: video.temporal_diff(t, s01, D_w, Y_w, slots, D_out, Y_out, slots, filt, out=out)
for f in forms.values():
    f(); f()
torch.cuda.synchronize()
samples = {k: [] for k in forms}
for _ in range(args.rounds):
    for k, f in forms.items():
        samples[k].append(timed(f))
nbytes = 4 * B * S * S * (3 + 3 + 1 + 3 + 1)
say(f'motion search: n {B} faces of one frame step, S {S}, every face with a previous frame; {nbytes / 1e6:.1f} MB moved per mkd_motion_warp call (counted from the shapes)')
say(f'us per call = device time between events around {args.iters} back-to-back calls / {args.iters}; median (min) over {args.rounds} rounds, forms alternated')
for k, v in samples.items():
    med = statistics.median(v)
    rate = f'  {nbytes / med / 1e6:7.1f} GB/s' if k.startswith('mkd_motion_warp') else ''
    say(f'    {k:60s} device {med * 1e3:10.1f} us ({min(v) * 1e3:.1f}){rate}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
