#!/usr/bin/env python
"""The in-library loop's extras against the plain loop: batch 8, 256x256, 50 DDIM steps, graph replay, forms alternated in one process.
Without guidance (prepared batch B): plain, plain again (the spread of the measurement), trace with log_every_t 10.  With guidance 9
(prepared batch 2B): guided, guided again, guided with guidance rescale phi 0.7.  Prints ms per call of each form per round, the medians,
the step-launch counts, and writes the same lines to profiles/exp_sample_extras.txt.  The latents are not decoded: the figures are the
sampling loops alone.  What is NOT measured here: image quality under the rescale - this repository has no pretrained weights."""
import argparse, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from oracle import sampler

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, default=256)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--log-every-t', type=int, default=10)
ap.add_argument('--phi', type=float, default=0.7)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_sample_extras.txt'))
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


eng = MkdEngine(NetConfig())
eng.init_random(0, norm_jitter=0.2)
B, R, h = args.batch, args.res, args.res // 8
g = torch.Generator().manual_seed(0)
hint = torch.rand(B, 6, R, R, generator=g).cuda()
ctx = torch.randn(B, 77, 768, generator=g).cuda()
uctx = torch.zeros(B, 77, 768).cuda()
x_T = torch.randn(B, 4, h, h, generator=g).cuda()
sch = sampler.Schedule().make_ddim(args.steps)
tabs = ([int(t) for t in sch.ddim_timesteps], sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
run = lambda cfg, **k: eng.sample(x_T, *tabs, cfg_scale=cfg, use_graph=True, **k)
GROUPS = {
    1.0: {'plain': {}, 'plain-again': {}, f'trace-L{args.log_every_t}': dict(want_trace=True, log_every_t=args.log_every_t)},
    9.0: {'guided': {}, 'guided-again': {}, f'guided-phi{args.phi}': dict(guidance_rescale=args.phi)},
}
say(f'# sampling-loop extras: batch {B}, {R}x{R}, {args.steps} DDIM steps, graph replay, {args.rounds} rounds, forms alternated; '
    f'{torch.cuda.get_device_name(0)}')
ms = {f: [] for grp in GROUPS.values() for f in grp}
for r in range(args.rounds):
    for cfg, forms in GROUPS.items():
        if cfg == 1.0:
            eng.prepare(hint, ctx)
        else:
            eng.prepare(torch.cat([hint, hint]), torch.cat([uctx, ctx]))
        names = list(forms)
        for f in names:                           # untimed: plans and graph captures after the re-prepare
            out = run(cfg, **forms[f])
            assert torch.isfinite(out[0] if isinstance(out, tuple) else out).all(), f
        for f in names[r % 3:] + names[:r % 3]:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run(cfg, **forms[f])
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            ms[f].append(dt)
            say(f'round {r} {f:16s}: {dt:8.2f} ms per call, {dt / args.steps:.4f} ms per step')
med = {f: statistics.median(v) for f, v in ms.items()}
for cfg, forms in GROUPS.items():
    names = list(forms)
    base = med[names[0]]
    for f in names:
        say(f'median {f:16s}: {med[f]:8.2f} ms per call, {med[f] / args.steps:.4f} ms per step, {100.0 * (med[f] - base) / base:+.2f} % of {names[0]}'
            f' (min {min(ms[f]):.2f}, max {max(ms[f]):.2f})')
say(f'step launches (graph replay): plain {eng.step_launches(True, False)}, guided {eng.step_launches(True, True)}, '
    f'guided with rescale {eng.step_launches(True, True, rescale=True)}')
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
eng.close()
