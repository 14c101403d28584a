#!/usr/bin/env python
"""The guided pastes against the bilinear ones at the photo workload: batch 8, a 1536^2 box (x 6) of a 2048 x 2048 photo, S 256, feather
8.  mkd_paste_photo_guided (radius 1 and 2, and 0 for the cost of the range weight alone) against mkd_paste_photo, and
mkd_paste_frame_guided against mkd_paste_frame on the same squares rolled by 17 degrees; one launch each.  A device sample is the time
between two events around --iters back-to-back calls (buffers allocated once, outside), divided by --iters, median (minimum) over
--rounds rounds; the forms of a comparison are alternated inside the rounds."""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import photo

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=5)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--box', type=int, default=1536)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--sigma', type=float, default=8.0)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_paste_guided.py measures on the GPU: there is none')

lines = []
B, S, SIDE, RHO = args.batch, args.size, args.box, 8
HW = SIDE + 512


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


def compare(forms):
    for f in forms.values():
        f(); f()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            samples[k].append(timed(f))
    for k, v in samples.items():
        say(f'    {k:44s} device {statistics.median(v) * 1e3:10.1f} us ({min(v) * 1e3:.1f})')
    return {k: statistics.median(v) for k, v in samples.items()}


g = torch.Generator().manual_seed(23)
work = [torch.randint(0, 256, (HW, HW, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
s01 = torch.rand((B, 3, S, S), generator=g).cuda()
t = (torch.rand((B, 3, S, S), generator=g) * 2.0 - 1.0).cuda()
boxes = [(256, 256, SIDE, SIDE)] * B
frames = [photo.frame_from_box(b, 17.0) for b in boxes]
guide = lambda R: photo.GuidedPaste(R, args.sigma)
say(f'guided paste: batch {B}, a {SIDE}^2 box of a {HW} x {HW} photo, S {S} (x {SIDE / S:g}), feather {RHO}, sigma {args.sigma:g}; '
    f'{B * SIDE * SIDE / 1e6:.1f} M photo pixels per call')
say(f'us per call = device time between events around {args.iters} back-to-back calls / {args.iters}; median (min) over {args.rounds} rounds, forms alternated')
say('boxes: mkd_paste_photo_guided against mkd_paste_photo (1 launch each)')
r = compare({'mkd_paste_photo': lambda: photo.paste_photos(work, boxes, t, s01, RHO),
             **{f'mkd_paste_photo_guided  R {R} ({(2 * R + 2) ** 2:2d} taps)': (lambda R=R: photo.paste_photos(work, boxes, t, s01, RHO, guided=guide(R))) for R in (0, 1, 2)}})
base = r['mkd_paste_photo']
say('    guided / bilinear (medians): ' + ', '.join(f'R {R}: {v / base:.1f}' for R, v in zip((0, 1, 2), list(r.values())[1:])))
say('frames rolled 17 degrees: mkd_paste_frame_guided against mkd_paste_frame (1 launch each)')
r = compare({'mkd_paste_frame': lambda: photo.paste_frames(work, frames, t, s01, RHO),
             **{f'mkd_paste_frame_guided  R {R} ({(2 * R + 2) ** 2:2d} taps)': (lambda R=R: photo.paste_frames(work, frames, t, s01, RHO, guided=guide(R))) for R in (0, 1, 2)}})
base = r['mkd_paste_frame']
say('    guided / bilinear (medians): ' + ', '.join(f'R {R}: {v / base:.1f}' for R, v in zip((0, 1, 2), list(r.values())[1:])))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
