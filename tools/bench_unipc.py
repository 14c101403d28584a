#!/usr/bin/env python
"""UniPC against DPM-Solver++ and DDIM sampling: log_results' two passes (plain, then guidance 9) at batch 8, 256x256 through the
samplers and the in-library graph loop, alternated in one process: DDIM, DPM-Solver++ and UniPC (order --order, with the corrector) at
--steps (50), and UniPC at --few (10).  Prints images/s of each form per round, their medians, ms per step of each and the
step-launch counts (equal for the three solvers).  The latents are not decoded: the figures are the sampling loops alone.  What is NOT
measured here: image quality - that a predictor-corrector of this kind gives a usable image in 8-10 evaluations is the literature's
claim for pretrained weights, which this repository does not have."""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd.config import create_model

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, default=256)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--few', type=int, default=10)
ap.add_argument('--order', type=int, default=2)
ap.add_argument('--rounds', type=int, default=6)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
model = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml')).cpu()
model.cuda(0)
model.engine.init_random(seed=0)
model.solver_order = args.order
B, R, h = args.batch, args.res, args.res // 8
g = torch.Generator().manual_seed(0)
hint = torch.rand(B, 6, R, R, generator=g).cuda()
ctx = torch.randn(B, 77, model.net_config.context_dim, generator=g).cuda()
uctx = torch.zeros(B, 77, model.net_config.context_dim).cuda()
x_T = torch.randn(B, 4, h, h, generator=g).cuda()
cond = {'c_concat': [hint], 'c_crossattn': [ctx]}
uc = {'c_concat': [hint], 'c_crossattn': [uctx]}
FORMS = {f'ddim-{args.steps}': ('ddim', args.steps), f'dpmpp-{args.steps}': ('dpmpp', args.steps),
         f'unipc-{args.steps}': ('unipc', args.steps), f'unipc-{args.few}': ('unipc', args.few)}


def passes(form):
    model.sampler, steps = FORMS[form]
    a, _ = model.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=steps, x_T=x_T)
    b, _ = model.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=steps, x_T=x_T, unconditional_guidance_scale=9.0,
                            unconditional_conditioning=uc)
    return a, b


launches = {}
for form in FORMS:
    a, b = passes(form)                      # warm-up: plans, graph captures
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), form
    launches[form] = (model.engine.step_launches(True, False), model.engine.step_launches(True, True))
names = list(FORMS)
sec = {f: [] for f in FORMS}
for r in range(args.rounds):
    k = r % len(names)
    for form in names[k:] + names[:k]:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        passes(form)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        sec[form].append(dt)
        print(f'round {r} {form:9s}: {B / dt:.3f} images/s ({dt * 1e3:.1f} ms)', flush=True)
base = None
for form in names:
    dt = statistics.median(sec[form])
    steps = FORMS[form][1]
    # (one log_results call = two passes of `steps` steps each; a guided step evaluates 2B samples)
    line = f'median {form:9s}: {B / dt:.3f} images/s, {dt * 1e3 / (2 * steps):.3f} ms per step (mean of the plain and the guided pass)'
    if base is None:
        base = dt
    else:
        line += f', x{base / dt:.3f} of {names[0]}'
    print(line)
print('step launches (plain, guidance): ' + ', '.join(f'{f} {launches[f]}' for f in names))
