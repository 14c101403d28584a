#!/usr/bin/env python
"""Per-sample requests in one batch against the uniform loop: batch 8, 256x256, graph replay, forms alternated in one process.
Without guidance (prepared batch B): uniform 50 steps, uniform again (the distance between the two is the spread of the measurement),
per-sample with every row at 50 steps, per-sample with rows at 20 / 50 mixed, and uniform 20 steps for scale.  With guidance (prepared
batch 2B): uniform guidance 9, again, per-sample with guidance 9 / 1.5 mixed.  Prints ms per call of each form per round, the medians,
the step-launch counts, and writes the same lines to profiles/exp_per_sample.txt.  Two expectations are checked by the reader of that
file: a per-sample step takes the uniform step's time within the uniform-against-uniform spread, and a mixed call takes the time of its
longest row.  The latents are not decoded: the figures are the sampling loops alone."""
import argparse, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from makeupdiffuse_amd.batching import SampleSpec, build_rows
from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from oracle import sampler

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, default=256)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--short', type=int, default=20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exp_per_sample.txt'))
args = ap.parse_args()
if args.rounds < 5:
    raise SystemExit('--rounds: at least 5 (the medians are over the rounds)')

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
AC = sampler.Schedule().alphas_cumprod
S, S2 = args.steps, args.short


def uniform(steps, cfg):
    row = build_rows([SampleSpec(steps)], AC)[0]
    return lambda: eng.sample(x_T, row.timesteps, row.alphas, row.alphas_prev, row.sqrt_one_minus_alphas, cfg_scale=cfg, use_graph=True)


def per_sample(specs):
    rows = build_rows(specs, AC)
    return lambda: eng.sample_rows(x_T, rows, use_graph=True)


mixed_steps = [SampleSpec(S2 if b % 2 == 0 else S) for b in range(B)]
mixed_scale = [SampleSpec(S, guidance=9.0 if b % 2 == 0 else 1.5) for b in range(B)]
GROUPS = {
    False: {f'uniform-{S}': (uniform(S, 1.0), S), f'uniform-{S}-again': (uniform(S, 1.0), S),
            f'rows-all-{S}': (per_sample([SampleSpec(S)] * B), S), f'rows-{S2}/{S}-mixed': (per_sample(mixed_steps), S),
            f'uniform-{S2}': (uniform(S2, 1.0), S2)},
    True: {'guided-9': (uniform(S, 9.0), S), 'guided-9-again': (uniform(S, 9.0), S),
           'rows-guided-9/1.5-mixed': (per_sample(mixed_scale), S)},
}
say(f'# per-sample requests in one batch: batch {B}, {R}x{R}, {S} DDIM steps (short rows {S2}), graph replay, {args.rounds} rounds, '
    f'forms alternated; {torch.cuda.get_device_name(0)}')
ms = {f: [] for grp in GROUPS.values() for f in grp}
for r in range(args.rounds):
    for guided, forms in GROUPS.items():
        if guided:
            eng.prepare(torch.cat([hint, hint]), torch.cat([uctx, ctx]))
        else:
            eng.prepare(hint, ctx)
        names = list(forms)
        for f in names:                           # untimed: plans and graph captures after the re-prepare
            assert torch.isfinite(forms[f][0]()).all(), f
        k = r % len(names)
        for f in names[k:] + names[:k]:
            forms[f][0]()                         # (the captured step is keyed on the form: re-captured untimed when the form changes)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            forms[f][0]()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            ms[f].append(dt)
            say(f'round {r} {f:26s}: {dt:8.2f} ms per call, {dt / forms[f][1]:.4f} ms per executed step')
med = {f: statistics.median(v) for f, v in ms.items()}
for guided, forms in GROUPS.items():
    names = list(forms)
    base = med[names[0]]
    for f in names:
        say(f'median {f:26s}: {med[f]:8.2f} ms per call, {med[f] / forms[f][1]:.4f} ms per executed step, '
            f'{100.0 * (med[f] - base) / base:+.2f} % of {names[0]} (min {min(ms[f]):.2f}, max {max(ms[f]):.2f})')
    say(f'spread ({names[0]} against {names[1]}): {100.0 * abs(med[names[1]] - base) / base:.2f} %')
say(f'step launches (graph replay): uniform {eng.step_launches(True, False)} / per-sample {eng.step_launches(True, False, per_sample=True)}, '
    f'guided {eng.step_launches(True, True)} / per-sample {eng.step_launches(True, True, per_sample=True)}')
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
eng.close()
