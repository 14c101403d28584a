#!/usr/bin/env python
"""The face-parsing network (mkd_parser_parse: images in, label maps out) at 512 x 512, batch 1 / 8 / 16, random weights: ms per
call, launches per call and the TFLOP/s that makes.  Every batch size runs in a child process of its own under its own time limit;
the first one that fails, or runs out of time, ends the run (nothing more is started on the device after it).  A sample is the
device time between two events around --iters back-to-back calls, divided by --iters; the table gives the median and the minimum
over --rounds rounds.  The log goes to profiles/exp_face_parser.txt (--out)."""
import argparse, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, nargs='+', default=[1, 8, 16])
ap.add_argument('--res', type=int, default=512)
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--limit', type=int, default=120, help='seconds each batch size may take')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_face_parser.txt'))
ap.add_argument('--child', type=int, default=0, help=argparse.SUPPRESS)
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')


def child(B):
    import torch
    from makeupdiffuse_amd.face_parser import FaceParser
    p = FaceParser().init_random(0).finalize()
    x = torch.rand(B, 3, args.res, args.res, generator=torch.Generator().manual_seed(B)).cuda()
    p.parse(x); torch.cuda.synchronize()          # first call: allocates the workspace
    samples = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            p.parse(x)
        b.record(); torch.cuda.synchronize()
        samples.append(a.elapsed_time(b) / args.iters)
    med, fl = statistics.median(samples), p.flops(args.res, args.res) * B
    print(f'batch {B:3d}  {args.res}x{args.res}  {med:8.3f} ms median ({min(samples):.3f} min)  {med / B:7.3f} ms per image  '
          f'{p.launches():3d} launches  {fl / 1e9:8.1f} GFLOP  {fl / med / 1e9:6.1f} TFLOP/s', flush=True)


if args.child:
    child(args.child)
    sys.exit(0)
lines = [f'mkd_parser_parse, random weights; ms per call = device time between events around {args.iters} back-to-back calls / {args.iters}; '
         f'median (min) over {args.rounds} rounds']
print(lines[0], flush=True)
for B in args.batch:
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(B), '--res', str(args.res), '--rounds', str(args.rounds),
                            '--iters', str(args.iters)], capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        lines.append(f'batch {B}: no result within {args.limit} s; stopping')
        print(lines[-1], flush=True)
        break
    text = r.stdout.strip() or r.stderr.strip()[-2000:]
    lines.append(text)
    print(text, flush=True)
    if r.returncode != 0:
        lines.append(f'batch {B}: exit status {r.returncode}; stopping')
        print(lines[-1], flush=True)
        break
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
