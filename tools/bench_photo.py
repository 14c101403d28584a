#!/usr/bin/env python
"""The two photo calls (mkd_crop_resize, mkd_paste_photo) at batch 8: a 2000^2 box of a 4000 x 3000 photo -> 256^2 and back, each timed
against what it replaces and never against itself:
  crop-resize: Pillow's Image.resize((S, S), BILINEAR, box=...) of every photo on the host plus the upload of the result (host clock
               around the loop and a device synchronise);
  paste:       the same arithmetic as a chain of torch operations on the device: F.interpolate(bilinear) of the difference, feather
               weights, add, round, clamp, uint8, written into the box.
The forms alternate inside every round of one process; a device sample is the time between two events around --iters back-to-back
calls, divided by --iters; the table gives the median and the minimum over --rounds rounds.  Each result is compared with its
baseline once: the resize must equal Pillow's bytes, the paste may differ from the torch chain by one grey level (the chain rounds
its interpolation differently)."""
import argparse, os, statistics, sys, time
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import photo

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--photo', type=int, nargs=2, default=[3000, 4000], metavar=('H', 'W'))
ap.add_argument('--box', type=int, nargs=4, default=[1000, 500, 2000, 2000], metavar=('X0', 'Y0', 'W', 'H'))
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--feather', type=int, default=8)
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_photo.py measures on the GPU: there is none')
from PIL import Image

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


B, (H, W), S, rho = args.batch, args.photo, args.size, args.feather
box = tuple(args.box)
x0, y0, bw, bh = box
g = torch.Generator(device='cuda').manual_seed(1)
smooth = F.interpolate(torch.rand(B, 3, H // 8, W // 8, device='cuda', generator=g), size=(H, W), mode='bilinear', align_corners=False)
photos_t = ((smooth + 0.1 * torch.rand(B, 3, H, W, device='cuda', generator=g)).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
del smooth
photos = list(photos_t.unbind(0))
host = [p.cpu().numpy() for p in photos]
boxes = [box] * B


def pil_resize():
    out = np.stack([np.asarray(Image.fromarray(h).resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + bw, y0 + bh)), dtype=np.float32) / 255.0
                    for h in host])
    return torch.from_numpy(out).permute(0, 3, 1, 2).contiguous().cuda()


def feather_weights():
    j, i = torch.arange(bw, device='cuda'), torch.arange(bh, device='cuda')
    big = torch.full((), 1 << 30, device='cuda')
    ex = torch.minimum(j if x0 > 0 else big.expand(bw), bw - 1 - j if x0 + bw < W else big.expand(bw))
    ey = torch.minimum(i if y0 > 0 else big.expand(bh), bh - 1 - i if y0 + bh < H else big.expand(bh))
    e = torch.minimum(ey[:, None], ex[None, :])
    return (torch.clamp(e + 1, max=rho + 1).float() / float(rho + 1))[None, None]


def torch_paste(dst, t, s01):
    d = ((t + 1.0) * 0.5 - s01) * 255.0
    u = F.interpolate(d, size=(bh, bw), mode='bilinear', align_corners=False)
    region = dst[:, y0:y0 + bh, x0:x0 + bw]
    o = region.permute(0, 3, 1, 2).float() + feather_weights() * u
    region.copy_(o.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1))


say(f'photo calls, batch {B}: box {bw}x{bh} at ({x0}, {y0}) of a {W}x{H} photo <-> {S}^2, feather {rho}; device forms: ms per call = device '
    f'time between events around {args.iters} back-to-back calls / {args.iters}; host form: wall clock around one call and a synchronise; '
    f'median (min) over {args.rounds} rounds, forms alternated within each round')
crop = photo.crop_resize(photos, boxes, S, want_u8=True)
ref = pil_resize()
same = bool(torch.equal(crop.img01, ref))
say(f'crop-resize against Pillow: {"the same bytes" if same else "DIFFERENT"}')
assert same
s01 = crop.img01
gt = torch.Generator(device='cuda').manual_seed(2)
t = (s01 * 2.0 - 1.0 + 0.3 * torch.randn(s01.shape, device='cuda', generator=gt)).clamp(-1, 1)
a, b = photos_t.clone(), photos_t.clone()
photo.paste_photos(list(a.unbind(0)), boxes, t, s01, rho)
torch_paste(b, t, s01)
diff = (a.int() - b.int()).abs()
say(f'paste against the torch chain: max difference {int(diff.max())} grey level(s), {100.0 * float((diff != 0).float().mean()):.3f} % of the bytes differ')
assert int(diff.max()) <= 1
outside = torch.ones(H, W, dtype=torch.bool, device='cuda')
outside[y0:y0 + bh, x0:x0 + bw] = False
assert torch.equal(a[:, outside], photos_t[:, outside])
del diff, outside, b

work = list(a.unbind(0))
device_forms = {'mkd_crop_resize (2 launches)': lambda: photo.crop_resize(photos, boxes, S),
                'mkd_paste_photo (1 launch)': lambda: photo.paste_photos(work, boxes, t, s01, rho),
                'torch chain of the paste': lambda: torch_paste(a, t, s01)}
host_forms = {'Pillow resize on the host + upload': pil_resize}
for fn in list(device_forms.values()) + list(host_forms.values()):
    fn(); fn()
torch.cuda.synchronize()
samples = {k: [] for k in list(device_forms) + list(host_forms)}
for _ in range(args.rounds):
    for k, fn in device_forms.items():
        samples[k].append(timed(fn))
    for k, fn in host_forms.items():
        samples[k].append(timed_host(fn))
moved = {'mkd_crop_resize (2 launches)': B * (bw * bh * 3 + 2 * bh * S * 3 + S * S * 3 * 4),
         'mkd_paste_photo (1 launch)': B * (2 * bw * bh * 3 + 2 * S * S * 3 * 4)}
for k, v in samples.items():
    med, best = statistics.median(v), min(v)
    extra = f'  {moved[k] / med * 1e-6:.0f} GB/s of the {moved[k] / 1e6:.1f} MB it must move' if k in moved else ''
    say(f'    {k:38s} {med:9.4f} ms ({best:.4f}){extra}')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
