#!/usr/bin/env python
"""The pixel-space background paste (mkd_paste_background) at batch 8, 256^2 and 512^2: the label path at feather 0, 4 and 16 and the
fp32-mask path, each ONE launch, timed against two references and never against itself:
  (a) mkd_decode of the same batch, the call the paste follows (is the launch a few percent of it?);
  (b) the same arithmetic as a chain of torch operations on the device: class test -> replicate pad -> avg_pool2d -> blend.
The forms alternate inside every round of one process; a sample is the device time between two events around --iters back-to-back
calls, divided by --iters; the table gives the median and the minimum over --rounds rounds.  The torch chain's result is compared with
the kernel's once (it is not bit-exact: avg_pool2d sums floats)."""
import argparse, ctypes as C, os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, VaeConfig

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
ap.add_argument('--feather', type=int, nargs='+', default=[0, 4, 16])
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')

CLASSES = (0, 11, 12)
eng = MkdEngine(NetConfig()); eng.configure_vae(VaeConfig()); eng.init_random(0)
lib, stream = eng.lib, lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def face_seg(B, res):
    """background around an ellipse of skin with hair on top and a strip of teeth: the classes the paste keeps cover about half"""
    yy, xx = torch.meshgrid(torch.arange(res, dtype=torch.float32), torch.arange(res, dtype=torch.float32), indexing='ij')
    seg = torch.zeros(B, res, res, dtype=torch.uint8)
    for b in range(B):
        cy, cx = res * (0.5 + 0.01 * b), res * (0.5 - 0.01 * b)
        inside = ((yy - cy) / (0.4 * res)) ** 2 + ((xx - cx) / (0.3 * res)) ** 2 <= 1.0
        seg[b][inside] = 1
        seg[b][inside & (yy < cy - 0.25 * res)] = 12
        seg[b][inside & ((yy - cy - 0.18 * res).abs() < 0.01 * res) & ((xx - cx).abs() < 0.06 * res)] = 11
    return seg


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


def torch_chain(image, src, seg, rho):
    keep = torch.zeros_like(seg, dtype=torch.bool)
    for c in CLASSES:
        keep |= seg == c
    a = keep.float().unsqueeze(1)
    if rho:
        a = F.avg_pool2d(F.pad(a, (rho, rho, rho, rho), mode='replicate'), 2 * rho + 1, stride=1)
    return ((a * ((src + 1) / 2) + (1 - a) * ((image + 1) / 2)) * 2.0 - 1.0).clamp(-1, 1)


B = args.batch
say(f'mkd_paste_background, batch {B}, 3 channels; ms per call = device time between events around {args.iters} back-to-back calls / '
    f'{args.iters}; median (min) over {args.rounds} rounds, forms alternated within each round')
for res in args.res:
    g = torch.Generator().manual_seed(res)
    image = (torch.rand(B, 3, res, res, generator=g) * 2.2 - 1.1).cuda()
    src = (torch.rand(B, 3, res, res, generator=g) * 2 - 1).cuda()
    seg = face_seg(B, res).cuda()
    mask = torch.rand(B, 1, res, res, generator=g).cuda()
    z = torch.randn(B, 4, res // 8, res // 8, generator=g).cuda()
    out = torch.empty_like(image)
    bits = sum(1 << c for c in CLASSES)
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())

    def kernel(labels, rho, m):
        rc = lib.mkd_paste_background(ptr(image), ptr(src), ptr(labels), C.c_uint64(bits), 1, rho, ptr(m), B, ptr(out), None, B, 3, res, res, stream())
        assert rc == 0, rc

    forms = {'mkd_decode (the call before it)': lambda: eng.decode(z)}
    for rho in args.feather:
        forms[f'paste, labels, feather {rho}'] = lambda rho=rho: kernel(seg, rho, None)
        forms[f'torch chain, feather {rho}'] = lambda rho=rho: torch_chain(image, src, seg, rho)
    forms['paste, fp32 mask'] = lambda: kernel(None, 0, mask)
    forms['torch blend of an fp32 mask'] = lambda: ((mask * ((src + 1) / 2) + (1 - mask) * ((image + 1) / 2)) * 2.0 - 1.0).clamp(-1, 1)
    for rho in args.feather:                                     # the two forms compute the same thing
        kernel(seg, rho, None)
        d = float((out - torch_chain(image, src, seg, rho)).abs().max())
        assert d <= 1e-5, (rho, d)
        say(f'{res}x{res} feather {rho}: max |kernel - torch chain| = {d:.2e}')
    for fn in forms.values():                                    # warm every form and shape
        fn(); fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            samples[k].append(timed(fn))
    dec = statistics.median(samples['mkd_decode (the call before it)'])
    moved = B * res * res * (3 * 3 * 4 + 1)                      # image + src + out fp32 and the label bytes
    say(f'{res}x{res}:')
    for k, v in samples.items():
        med, best = statistics.median(v), min(v)
        extra = ''
        if k.startswith('paste'):
            extra = f'  {100 * med / dec:.2f} % of the decode, {moved / med * 1e-6:.0f} GB/s of the {moved / 1e6:.1f} MB it must move'
        say(f'    {k:34s} {med:8.4f} ms ({best:.4f}){extra}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
