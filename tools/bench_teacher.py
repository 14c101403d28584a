#!/usr/bin/env python
"""The histogram-matching teacher at n = 8 pairs of S = 256: teacher.pseudo_ground_truth (region masks of both label maps, ONE
mkd_hist_match for the tables, ONE mkd_pgt_compose), the compose launch alone on prepared masks and tables, and the same x_p composed
from torch ops on mkd_hist_match's matched images (feather 0: a chain of torch.where; feather > 0: box-filtered one-hot planes and a
gather of the tables), each at feather 0, 2 and 8.  A device sample is the time between two events around --iters back-to-back calls,
divided by --iters, median (minimum) over --rounds rounds; the forms are alternated inside the rounds.  --model: also a full
log_results (plain + guided pass, --steps steps) on the randomly initialised model of runs/test.py against the same call with
teacher_start = --tau, wall time around a device synchronisation.  --warp: also the landmark-warped term at K = 68 landmarks per pair:
mkd_pgt_warp alone (feather 0, 2, 8), the same image composed from torch ops on the device (the thin-plate spline in float64, grid_sample
for the colours and the reference masks, box-filtered one-hot planes for the weights) and pseudo_ground_truth whole with and without
warp, in the same median-of-rounds form.  --points: also the control points from the region masks and the spline solve on the device
(D = 16 directions, K = 68 pairs): mkd_region_points alone on the [4, 2 n] masks, mkd_tps_solve alone on those points and on 68 random
landmarks, pseudo_ground_truth whole with the host solve, with the device solve and with mask points, and the largest difference between
the maps of the device solve and of the host solve."""
import argparse, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import teacher_ref as tr
from makeupdiffuse_amd import makeup_score as ms
from makeupdiffuse_amd import teacher

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--model', action='store_true', help='also time a sampling pass with and without teacher_start')
ap.add_argument('--warp', action='store_true', help='also time the landmark-warped term (mkd_pgt_warp) against a torch composition')
ap.add_argument('--points', action='store_true', help='also time mkd_region_points, mkd_tps_solve and the warped teacher with the device solve / mask points')
ap.add_argument('--landmarks', type=int, default=68)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--tau', type=float, default=0.6)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_teacher.py measures on the GPU: there is none')

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


src, ref, sseg, rseg = (torch.from_numpy(x).cuda() for x in tr.synthetic_pairs(n=B, size=S))
_, tables, counts = teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=0)
masks = torch.stack([ms.region_masks(sseg)[0][r] for r in ms.REGIONS]).contiguous()          # [4, B, S, S]
rmasks = torch.stack([ms.region_masks(rseg)[0][r] for r in ms.REGIONS]).contiguous()
matched = ms.histogram_match(src.repeat(4, 1, 1, 1), ref.repeat(4, 1, 1, 1), masks.view(4 * B, S, S), rmasks.view(4 * B, S, S), want_loss=False)[0]
matched = matched.view(4, B, 3, S, S)
out = torch.empty_like(src)
ORDER = (1, 3, 2, 0)          # skin, eye_right, eye_left, lip: the highest priority is written last


def torch_hard():
    """feather 0 from the matched images: inside region r (by priority) matched_r + the source's sub-bin fraction, else the source"""
    v = src.clamp(0, 1) * 255.0
    x = v
    frac = v - v.floor()
    for r in ORDER:
        x = torch.where(masks[r][:, None] != 0, matched[r] + frac, x)
    return (x / 255.0).clamp(0, 1)


def torch_soft(F):
    v = src.clamp(0, 1) * 255.0
    i = v.long().clamp(max=255)
    ids = torch.zeros_like(masks[0])
    for r, rid in zip(ORDER, (4, 3, 2, 1)):
        ids = torch.where(masks[r] != 0, torch.full_like(ids, rid), ids)
    acc = v
    for plane, rid in ((0, 1), (2, 2), (3, 3), (1, 4)):
        w = torch.nn.functional.avg_pool2d((ids == rid).float()[:, None], 2 * F + 1, 1, F, count_include_pad=True)
        T = torch.gather(tables[plane].float(), 2, i.view(B, 3, S * S)).view(B, 3, S, S)
        acc = acc + w * (T - i)
    return (acc / 255.0).clamp(0, 1)


assert torch.equal(teacher.compose(src, masks, tables, None, 0), teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=0)[0])
err = (torch_hard() - teacher.compose(src, masks, tables, None, 0)).abs().max().item()
err2 = (torch_soft(2) - teacher.compose(src, masks, tables, None, 2)).abs().max().item()
say(f'n = {B}, S = {S}: region pixels of pair 0 (source, reference) {counts[:, 0].tolist()}; torch compositions differ from mkd_pgt_compose by at '
    f'most {err:.2e} (feather 0) / {err2:.2e} (feather 2): fp32 against one rounding of a double')
forms = {}
for F in (0, 2, 8):
    forms[f'teacher.pseudo_ground_truth      feather {F} ({teacher.launches()} launches)'] = lambda F=F: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=F)
    forms[f'mkd_pgt_compose alone            feather {F} (1 launch)'] = lambda F=F: teacher.compose(src, masks, tables, None, F, out=out)
    forms[f'torch composition alone          feather {F}'] = torch_hard if F == 0 else (lambda F=F: torch_soft(F))
for call in forms.values():
    call()
torch.cuda.synchronize()
samples = {k: [] for k in forms}
for _ in range(args.rounds):
    for k, call in forms.items():
        samples[k].append(timed(call))
for k, v in samples.items():
    say(f'{k}: median {statistics.median(v) * 1e3:8.1f} us, min {min(v) * 1e3:8.1f} us')

if args.warp:
    import numpy as np
    K = args.landmarks
    rng = np.random.RandomState(0)
    flat = np.stack([rng.choice(S * S, K, replace=False) for _ in range(B)])
    lms_s = np.stack([flat // S, flat % S], 2).astype(np.float64)
    lms_r = lms_s + rng.uniform(-S / 16, S / 16, lms_s.shape)
    ctrl_h, coef_h, kcount_h = teacher.tps_coefficients(lms_s, lms_r)
    ctrl, coef, kcount = (torch.from_numpy(a).cuda() for a in (ctrl_h, coef_h, kcount_h))
    alphas = teacher.alpha_rows(True, B).cuda()
    xh = teacher.compose(src, masks, tables, None, 2)
    wout = torch.empty_like(src)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float64, device='cuda'), torch.arange(S, dtype=torch.float64, device='cuda'), indexing='ij')

    def torch_warp(F):
        d2 = (yy - ctrl[:, :, 0, None, None]) ** 2 + (xx - ctrl[:, :, 1, None, None]) ** 2                      # [B, K, S, S]
        U = torch.where(d2 > 0, d2 * torch.log(d2), torch.zeros_like(d2))
        q = (coef[:, :, :K, None, None] * U[:, None]).sum(2) + coef[:, :, K, None, None] + coef[:, :, K + 1, None, None] * yy + coef[:, :, K + 2, None, None] * xx
        grid = torch.stack([2 * q[:, 1] / (S - 1) - 1, 2 * q[:, 0] / (S - 1) - 1], -1).float()
        R = torch.nn.functional.grid_sample(ref.clamp(0, 1), grid, mode='bilinear', padding_mode='border', align_corners=True)
        ids = torch.zeros_like(masks[0])
        for r, rid in zip(ORDER, (4, 3, 2, 1)):
            ids = torch.where(masks[r] != 0, torch.full_like(ids, rid), ids)
        Wt = torch.zeros(B, 1, S, S, device='cuda')
        for plane, rid in ((0, 1), (2, 2), (3, 3), (1, 4)):
            w = torch.nn.functional.avg_pool2d((ids == rid).float()[:, None], 2 * F + 1, 1, F, count_include_pad=True)
            mr = torch.nn.functional.grid_sample((rmasks[plane] != 0).float()[:, None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)
            Wt = Wt + alphas[:, plane, None, None, None] * w * mr
        Wt = Wt.clamp(max=1.0)
        return xh + Wt * (R - xh)

    errw = (torch_warp(2) - teacher.warp_blend(xh, ref, masks, rmasks, ctrl, coef, kcount, alphas, 2)).abs().max().item()
    say(f'warp, K = {K} landmarks per pair displaced by up to S / 16: the torch composition differs from mkd_pgt_warp by at most {errw:.2e} (feather 2): an '
        f'fp32 sampling grid against positions and blends in double')
    wforms = {}
    for F in (0, 2, 8):
        wforms[f'mkd_pgt_warp alone               feather {F} (1 launch)'] = lambda F=F: teacher.warp_blend(xh, ref, masks, rmasks, ctrl, coef, kcount, alphas, F, out=wout)
        wforms[f'torch warp composition alone     feather {F}'] = lambda F=F: torch_warp(F)
    wforms[f'teacher.pseudo_ground_truth      feather 2, no warp ({teacher.launches()} launches)'] = lambda: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=2)
    wforms[f'teacher.pseudo_ground_truth      feather 2, warp ({teacher.launches(warp=True)} launches, host solve + 3 uploads)'] = \
        lambda: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=2, lms_src=lms_s, lms_ref=lms_r, warp=True)
    for call in wforms.values():
        call()
    torch.cuda.synchronize()
    wsamples = {k: [] for k in wforms}
    for _ in range(args.rounds):
        for k, call in wforms.items():
            wsamples[k].append(timed(call))
    for k, v in wsamples.items():
        say(f'{k}: median {statistics.median(v) * 1e3:8.1f} us, min {min(v) * 1e3:8.1f} us')
    t0 = time.perf_counter()
    for _ in range(10):
        teacher.tps_coefficients(lms_s, lms_r)
    say(f'teacher.tps_coefficients on the host, {B} systems of {K + 3}^2: {(time.perf_counter() - t0) * 100:.2f} ms per call')

if args.points:
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import teacher_points_ref as pr
    K = 68
    rng = np.random.RandomState(0)
    flat = np.stack([rng.choice(S * S, K, replace=False) for _ in range(B)])
    lms_s = np.stack([flat // S, flat % S], 2).astype(np.float64)
    lms_r = lms_s + rng.uniform(-S / 16, S / 16, lms_s.shape)
    both = torch.cat([masks, rmasks], 1).contiguous()          # [4, 2 B, S, S]: [region][src | ref], what pseudo_ground_truth has
    pts, use, count = teacher.region_points(both, 16)
    want = pr.region_points_ref(both.cpu().numpy(), 16)
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((pts, use, count), want)), 'mkd_region_points differs from the restatement'
    ps, pf, us, uf = pts[:B].contiguous(), pts[B:].contiguous(), use[:B].contiguous(), use[B:].contiguous()
    kc_m = teacher.tps_coefficients_device(ps, pf, us, uf)[2].tolist()
    ls, lr = torch.from_numpy(lms_s).cuda(), torch.from_numpy(lms_r).cuda()
    dev = teacher.tps_coefficients_device(ls, lr)
    host = teacher.tps_coefficients(lms_s, lms_r)
    assert dev[2].tolist() == host[2].tolist() and dev[0].cpu().numpy().tobytes() == host[0].tobytes()
    zero, none = torch.zeros_like(src), torch.zeros_like(masks)
    qmap = lambda c, f, k: teacher.warp_blend(zero, zero, none, none, c, f, k, torch.ones(B, 4, device='cuda'), want_map=True)[1]
    diff = (qmap(*dev) - qmap(*(torch.from_numpy(a).cuda() for a in host))).abs().max().item()
    say(f'points, n = {B} pairs at {S}^2, D = 16: region pixels of image 0 (lip, eye_left, eye_right, skin) {count[0].tolist()}; control points kept per pair '
        f'from the masks {kc_m} of {K}; mkd_region_points equals the numpy restatement byte for byte')
    say(f'{K} random landmarks per pair displaced by up to S / 16: ctrl and kcount of mkd_tps_solve equal the host solve bit for bit; its map differs from the '
        f"host solve's by at most {diff:.3e} px over all {S}^2 pixels (Delta_ref of the tests, two host solves against each other: {pr.delta_ref():.3e} px)")
    L3 = teacher.launches
    pforms = {
        f'mkd_region_points alone          {2 * B} images (3 launches)': lambda: teacher.region_points(both, 16),
        f'mkd_tps_solve alone              mask points, K = {K} (1 launch)': lambda: teacher.tps_coefficients_device(ps, pf, us, uf),
        f'mkd_tps_solve alone              landmarks, K = {K} (1 launch)': lambda: teacher.tps_coefficients_device(ls, lr),
        f'teacher.pseudo_ground_truth      feather 2, warp, host solve ({L3(warp=True)} launches + 3 uploads)':
            lambda: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=2, lms_src=lms_s, lms_ref=lms_r, warp=True),
        f"teacher.pseudo_ground_truth      feather 2, warp, device solve ({L3(warp=True, solve='device')} launches + 2 uploads)":
            lambda: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=2, lms_src=lms_s, lms_ref=lms_r, warp=True, solve='device'),
        f"teacher.pseudo_ground_truth      feather 2, warp, mask points ({L3(warp=True, points='masks')} launches + 1 upload)":
            lambda: teacher.pseudo_ground_truth(src, ref, sseg, rseg, feather=2, warp=True, points='masks'),
    }
    for call in pforms.values():
        call()
    torch.cuda.synchronize()
    psamples = {k: [] for k in pforms}
    for _ in range(args.rounds):
        for k, call in pforms.items():
            psamples[k].append(timed(call))
    for k, v in psamples.items():
        say(f'{k}: median {statistics.median(v) * 1e3:8.1f} us, min {min(v) * 1e3:8.1f} us')
    say('(the warped teacher with the host solve was measured at 1563 us per call when it was added: profiles/exp_teacher_warp.txt)')

if args.model:
    from makeupdiffuse_amd.config import create_model
    m = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml')).cpu()
    m.first_stage_encoder = True
    m.ddim_steps, m.teacher, m.save_images = args.steps, 'hist', False
    m.cuda(0)
    m.engine.init_random(seed=0)
    m.uncond_embedding = torch.zeros(1, 77, m.net_config.context_dim)
    batch = {'src_img': src.cpu(), 'ref_img': ref.cpu(), m.seg_key: sseg.cpu(), m.ref_seg_key: rseg.cpu(),
             'txt_emb': torch.randn(B, 77, m.net_config.context_dim, generator=torch.Generator().manual_seed(3))}
    wall = {None: [], args.tau: []}
    for rnd in range(4):          # the first round warms up (plans, graphs) and is dropped
        for tau in wall:
            m.teacher_start = tau
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.log_results(dict(batch), 0, seeds=1)
            torch.cuda.synchronize()
            if rnd:
                wall[tau].append(time.perf_counter() - t0)
    k = teacher.start_steps(args.tau, args.steps)
    say(f'log_results, batch {B} at {S}^2, plain + guided pass with the teacher rows: {args.steps} steps median {statistics.median(wall[None]) * 1e3:.1f} ms; '
        f'teacher_start = {args.tau} ({k} steps) median {statistics.median(wall[args.tau]) * 1e3:.1f} ms (3 rounds each, alternated)')
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
