#!/usr/bin/env python
"""Masked (background-preserving, DDIMSampler mask / x0) against unmasked sampling: log_results' two passes (plain, then guidance 9)
at batch 8, 256x256, 50 DDIM steps through DDIMSampler and the in-library graph loop, alternated in one process.  Prints images/s of
each form per round, their medians and the step-launch counts (masked and unmasked must be equal)."""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd.config import create_model

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, default=256)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--rounds', type=int, default=6)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
model = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml')).cpu()
model.cuda(0)
model.engine.init_random(seed=0)
B, R, h = args.batch, args.res, args.res // 8
g = torch.Generator().manual_seed(0)
hint = torch.rand(B, 6, R, R, generator=g).cuda()
ctx = torch.randn(B, 77, model.net_config.context_dim, generator=g).cuda()
uctx = torch.zeros(B, 77, model.net_config.context_dim).cuda()
x_T = torch.randn(B, 4, h, h, generator=g).cuda()
x0 = torch.randn(B, 4, h, h, generator=g).cuda()
mask = (torch.rand(B, 1, h, h, generator=g) > 0.5).float().cuda()
cond = {'c_concat': [hint], 'c_crossattn': [ctx]}
uc = {'c_concat': [hint], 'c_crossattn': [uctx]}


def passes(masked):
    kw = dict(x0=x0, mask=mask) if masked else {}
    model.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=args.steps, x_T=x_T, **kw)
    model.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=args.steps, x_T=x_T, unconditional_guidance_scale=9.0,
                     unconditional_conditioning=uc, **kw)


launches = {}
for masked in (False, True):
    passes(masked)                      # warm-up: plans, graph captures
    launches[masked] = (model.engine.step_launches(True, False), model.engine.step_launches(True, True))
rate = {False: [], True: []}
for r in range(args.rounds):
    for masked in ((False, True) if r % 2 == 0 else (True, False)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        passes(masked)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        rate[masked].append(B / dt)      # images of one log_results call (both passes) per second
        print(f'round {r} {"masked  " if masked else "unmasked"}: {B / dt:.3f} images/s ({dt * 1e3:.1f} ms)', flush=True)
mu, mm = statistics.median(rate[False]), statistics.median(rate[True])
print(f'median unmasked {mu:.3f} images/s, masked {mm:.3f} images/s ({(mm / mu - 1) * 100:+.2f} %)')
print(f'step launches (plain, guidance): unmasked {launches[False]}, masked {launches[True]}')
