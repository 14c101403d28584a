#!/usr/bin/env python
"""What a region-wise transfer from R references costs against the single-reference path: batch 8, 256x256, the prepare call
(mkd_prepare for R = 1, mkd_prepare_interp for R = 2, mkd_prepare_regions for R = 3 and 5) and the 50-step in-library graph loop
after each, forms alternated in one process, median of several rounds.  R = 1 is measured twice per round ('R1' and 'R1 again'):
the distance between those two is the run-to-run spread the other forms are read against.  A prepare is timed on its second call
after the form changed (the first one re-plans), the loop on its second run (the first one captures the step graph)."""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from makeupdiffuse_amd.schedule import DDIMSchedule

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, default=256)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--prepare-reps', type=int, default=5)
args = ap.parse_args()

eng = MkdEngine(NetConfig())
eng.init_random(seed=0)
B, h = args.batch, args.res // 8
g = torch.Generator().manual_seed(0)
src = torch.rand(B, 3, args.res, args.res, generator=g)
hints = [torch.cat((src, torch.rand(B, 3, args.res, args.res, generator=g)), 1).cuda() for _ in range(5)]
ctx = torch.randn(B, 77, eng.cfg.context_dim, generator=g).cuda()
x_T = torch.randn(B, 4, h, h, generator=g).cuda()
alpha = torch.rand(B, generator=g).cuda()
weights = {R: torch.softmax(torch.randn(B, R, h, h, generator=g), 1).cuda() for R in (3, 5)}
sch = DDIMSchedule().make_ddim(args.steps)
tables = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)

FORMS = {
    'R1': lambda: eng.prepare(hints[0], ctx),
    'R1 again': lambda: eng.prepare(hints[0], ctx),
    'R2 interp': lambda: eng.prepare(hints[0], ctx, hint2=hints[1], alpha=alpha),
    'R3 regions': lambda: eng.prepare_regions(hints[:3], weights[3], ctx),
    'R5 regions': lambda: eng.prepare_regions(hints[:5], weights[5], ctx),
}


def timed(fn, reps=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


prep = {k: [] for k in FORMS}
step = {k: [] for k in FORMS}
launches = {}
names = list(FORMS)
for r in range(args.rounds):
    for k in (names if r % 2 == 0 else names[::-1]):
        eng.prepare(None, ctx, latent_hw=(h, h))              # another plan in between: every form starts from a re-plan
        FORMS[k]()                                            # re-plans
        prep[k].append(timed(FORMS[k], args.prepare_reps))
        run = lambda: eng.sample(x_T, *tables, use_graph=True)
        run()                                                 # captures the step graph
        step[k].append(timed(run) / args.steps)
        launches[k] = (eng.step_launches(True, False), eng.eps_launches())
        print(f'round {r} {k:10s}: prepare {prep[k][-1]:.3f} ms, loop {step[k][-1]:.4f} ms/step', flush=True)
base_p, base_s = statistics.median(prep['R1']), statistics.median(step['R1'])
for k in names:
    p, s = statistics.median(prep[k]), statistics.median(step[k])
    print(f'median {k:10s}: prepare {p:.3f} ms ({p - base_p:+.3f} ms against R1), loop {s:.4f} ms/step ({(s / base_s - 1) * 100:+.2f} %), '
          f'step launches {launches[k][0]}, eps launches {launches[k][1]}')
eng.close()
