#!/usr/bin/env python
"""The makeup score on the device: 8 pairs x 8 histogram-matching terms (makeup_score.makeup_hist_terms: four region-mask calls over both label maps
and ONE mkd_hist_match call) at 256^2 and 512^2, device time between events, and mkd_hist_match alone on prepared masks with the launch
count the library reports for it (independent of n).  --reference-cpu: the same terms through the CPU restatement (tests/hist_match_ref.py), once, for scale.
The inputs are synthetic face layouts with different tone curves on the two sides."""
import argparse, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import makeup_score as ms

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=8)
ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--reference-cpu', action='store_true')
args = ap.parse_args()


def face_seg(res, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:res, 0:res].astype(np.float64)
    cy, cx = res * (0.5 + 0.03 * g.standard_normal()), res * (0.5 + 0.03 * g.standard_normal())
    ell = lambda dy, dx, ry, rx: ((yy - cy - dy * res) / (ry * res)) ** 2 + ((xx - cx - dx * res) / (rx * res)) ** 2 <= 1.0
    seg = np.zeros((res, res), np.uint8)
    seg[ell(0.3, 0, 0.15, 0.15)] = 13
    seg[ell(0, 0, 0.36, 0.29)] = 1
    seg[ell(0.02, 0, 0.07, 0.03)] = 6
    seg[ell(-0.09, -0.11, 0.03, 0.05)] = 4
    seg[ell(-0.09, 0.11, 0.03, 0.05)] = 5
    seg[ell(0.18, 0, 0.04, 0.09)] = 7
    seg[ell(0.18, 0, 0.04, 0.09) & (yy > cy + 0.18 * res)] = 9
    return seg


def timed(fn, iters):
    fn(); torch.cuda.synchronize()
    ms_ = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms_.append(a.elapsed_time(b))
    return statistics.median(ms_), min(ms_)


lib = mlib.load()
B = args.pairs
for res in args.res:
    g = torch.Generator().manual_seed(res)
    SR, RS = torch.rand(B, 3, res, res, generator=g) ** 2, 0.3 + 0.6 * torch.rand(B, 3, res, res, generator=g)
    S, R = torch.rand(B, 3, res, res, generator=g), torch.rand(B, 3, res, res, generator=g) ** 0.5
    src_seg = np.stack([face_seg(res, 10 + b) for b in range(B)])
    ref_seg = np.stack([face_seg(res, 50 + b) for b in range(B)])
    d = [t.cuda() for t in (SR, RS, S, R)] + [torch.from_numpy(src_seg).cuda(), torch.from_numpy(ref_seg).cuda()]
    med, best = timed(lambda: ms.makeup_hist_terms(*d), args.iters)
    out = ms.makeup_hist_terms(*d)
    print(f'{res}x{res}, {B} pairs x 8 terms: makeup_hist_terms (4 region-mask calls over both label maps + 1 mkd_hist_match) median {med:.3f} ms, min {best:.3f} ms; '
          f'skin pixels per pair ~{int(out["counts"][2, :, 0].float().mean())}, loss_makeup[0] {float(out["loss_makeup"][0]):.4f}')
    imgs = torch.cat(d[:2] + [d[3], d[2]])
    masks, _ = ms._region_masks_packed(torch.cat(d[4:]), ms.LIP_CLASSES, ms.SKIN_CLASSES, ms.FACE_CLASSES, ms.EYE_LEFT_CLASSES,
                                       ms.EYE_RIGHT_CLASSES, ms.EYE_MARGIN)
    flat, idx = masks.view(8 * B, res, res), ms._term_index(B, imgs.device)
    for want_matched in (False, True):
        med, best = timed(lambda: ms.histogram_match(imgs, imgs, flat, flat, index=idx, want_matched=want_matched), args.iters)
        print(f'    mkd_hist_match alone, n = {8 * B}, matched image {"written" if want_matched else "not written"}: median {med:.3f} ms, '
              f'min {best:.3f} ms, {lib.mkd_hist_match_launches(int(want_matched), 1)} launches for any n (as the library reports, not counted from the run)')
    if args.reference_cpu:
        import hist_match_ref as href
        t0 = time.perf_counter()
        for b in range(B):
            href.makeup_terms(SR[b].numpy(), RS[b].numpy(), S[b].numpy(), R[b].numpy(), src_seg[b], ref_seg[b])
        print(f'    CPU restatement (numpy, one thread of the host), the same {8 * B} terms: {(time.perf_counter() - t0) * 1e3:.1f} ms')
