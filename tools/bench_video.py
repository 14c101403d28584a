#!/usr/bin/env python
"""mkd_temporal_diff at the video workload: n = 8 faces of one frame step at S = 256, every face with a previous frame, window radius 0, 1
and 2; one launch each, the pools ping-ponged between calls as a clip does.  For scale, the bilinear and the guided paste of the same
8 faces into 1536^2 boxes (the call the filter sits in front of).  A device sample is the time between two events around --iters
back-to-back calls (buffers allocated once, outside), divided by --iters, median (minimum) over --rounds rounds; the forms are
alternated inside the rounds.  Bytes per call are counted from the shapes: t, s01 and D_in read, Y_in read, t_out, D_out and Y_out
written, all fp32."""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import photo, video

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=50)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--box', type=int, default=1536)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_video.py measures on the GPU: there is none')

lines = []
B, S, SIDE = args.batch, args.size, args.box


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


g = torch.Generator().manual_seed(29)
s01 = (torch.randint(0, 256, (B, 3, S, S), generator=g).float() / 255.0).cuda()
t = (torch.rand((B, 3, S, S), generator=g) * 2.0 - 1.0).cuda()
out = torch.empty_like(t)
pools = [(torch.zeros((B, 3, S, S), device='cuda'), torch.zeros((B, S, S), device='cuda')) for _ in range(2)]
slots = list(range(B))
turn = [0]


def step(filt):
    (Di, Yi), (Do, Yo) = pools[turn[0]], pools[1 - turn[0]]
    video.temporal_diff(t, s01, Di, Yi, slots, Do, Yo, slots, filt, out=out)
    turn[0] ^= 1


forms = {f'mkd_temporal_diff  R {R} ({(2 * R + 1) ** 2:2d} taps)': (lambda f=video.TemporalFilter(0.8, 4.0, R): step(f)) for R in (0, 1, 2)}
HW = SIDE + 512
work = [torch.randint(0, 256, (HW, HW, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
boxes = [(256, 256, SIDE, SIDE)] * B
forms['mkd_paste_photo (for scale)'] = lambda: photo.paste_photos(work, boxes, t, s01, 8)
forms['mkd_paste_photo_guided  R 1 (for scale)'] = lambda: photo.paste_photos(work, boxes, t, s01, 8, guided=photo.GuidedPaste(1, 8.0))
for f in forms.values():
    f(); f()
torch.cuda.synchronize()
samples = {k: [] for k in forms}
for _ in range(args.rounds):
    for k, f in forms.items():
        samples[k].append(timed(f))
nbytes = 4 * B * S * S * (3 * 3 + 1 + 3 * 2 + 1)
say(f'temporal filter: n {B} faces of one frame step, S {S}, every face with a previous frame; {nbytes / 1e6:.1f} MB moved per call (counted from the shapes)')
say(f'us per call = device time between events around {args.iters} back-to-back calls / {args.iters}; median (min) over {args.rounds} rounds, forms alternated')
for k, v in samples.items():
    med = statistics.median(v)
    rate = f'  {nbytes / med / 1e6:7.1f} GB/s' if k.startswith('mkd_temporal_diff') else ''
    say(f'    {k:44s} device {med * 1e3:10.1f} us ({min(v) * 1e3:.1f}){rate}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
