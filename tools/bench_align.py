#!/usr/bin/env python
"""The three tilted-face calls at the group-photo workload: 4 faces (rolled 25, -35, 12 and -20 degrees) in a 1536 x 1024 photo, S 256,
parse size 512.  mkd_crop_frame against mkd_crop_resize, mkd_paste_frame against mkd_paste_photo (plain, and both with a 512^2 weight
plane per face), and mkd_face_frames (four launches; table of 4 rows and of 64, as with own_pixels) next to mkd_label_components, the
call whose table it extends.  The frames are what the path itself makes of the map (label_components -> face_frames -> photo.grow_frame);
the axis-aligned forms take the boxes find_faces gives the same components.  A device sample is the time between two events around
--iters back-to-back calls (buffers allocated once, outside), divided by --iters, median (minimum) over --rounds rounds; the forms of a
comparison are alternated inside the rounds."""
import argparse, ctypes as C, math, os, statistics, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd import components, face_parser as fp, lib as mlib, photo

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default=None, help='also write the report to this file')
args = ap.parse_args()
if args.rounds < 6:
    raise SystemExit('--rounds must be at least 6 (the median of fewer says little)')
if not torch.cuda.is_available():
    raise SystemExit('bench_align.py measures on the GPU: there is none')

lines = []
P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
lib = mlib.load()
H, W, S, PS, RHO = 1024, 1536, 256, 512, 8
FACES = ((120, 150, 40, 52, 25.0), (260, 170, 36, 48, -35.0), (390, 330, 34, 44, 12.0), (150, 360, 30, 40, -20.0))          # cx, cy, rx, ry, roll on the map


def say(text):
    print(text, flush=True)
    lines.append(text)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        call()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


def report(samples):
    return f'{statistics.median(samples):8.4f} ms ({min(samples):.4f})'


def compare(forms):
    for f in forms.values():
        f(); f()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            samples[k].append(timed(f))
    for k, v in samples.items():
        say(f'    {k:44s} device {report(v)}')
    return {k: statistics.median(v) for k, v in samples.items()}


def face_map():
    """skin ellipses with two eye discs each (LUT_SEG 1, 4, 5), rolled about their centres"""
    y, x = np.mgrid[0:PS, 0:PS].astype(np.float64)
    lab = np.zeros((PS, PS), np.uint8)
    for cx, cy, rx, ry, roll in FACES:
        c, s = math.cos(math.radians(roll)), math.sin(math.radians(roll))
        u, v = c * (x + 0.5 - cx) + s * (y + 0.5 - cy), -s * (x + 0.5 - cx) + c * (y + 0.5 - cy)
        lab[(u / rx) ** 2 + (v / ry) ** 2 <= 1.0] = 1
        for eu, l in ((-0.4 * rx, 4), (0.4 * rx, 5)):
            lab[(u - eu) ** 2 + (v + 0.25 * ry) ** 2 <= (0.2 * rx) ** 2] = l
    return lab


labels = torch.from_numpy(face_map()[None]).cuda()
g = torch.Generator().manual_seed(11)
base_photo = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
table, count, ids = components.label_components(labels, fp.FACE_CLASSES, min_area=(PS // 32) ** 2, max_out=4, want_ids=True)
rows = components.face_frames(labels, ids, table, [(H, W)]).cpu().tolist()[0]
trow = table.cpu().tolist()[0]
assert int(count.item()) == 4
frames = [photo.grow_frame(r, PS, H, W) for r in rows]
boxes = [photo.grow_square_box((t[2] * H // PS, min(H, -(-(t[3] + 1) * H // PS)) - 1, t[4] * W // PS, min(W, -(-(t[5] + 1) * W // PS)) - 1), H, W) for t in trow]
say(f'group-photo workload: {len(frames)} faces of a {W} x {H} photo, S {S}, parse size {PS}; measured rolls '
    f'{[round(photo.frame_roll(r), 1) for r in rows]} degrees, frame sides {[round(f.side) for f in frames]}, box sides {[b[2] for b in boxes]} photo pixels')
say(f'ms per call = device time between events around {args.iters} back-to-back calls / {args.iters}; median (min) over {args.rounds} rounds, forms alternated')

copies = [base_photo.clone() for _ in frames]
say('crop: mkd_crop_frame (1 launch) against mkd_crop_resize (2 launches), img01 only')
r = compare({'mkd_crop_resize  (boxes)': lambda: photo.crop_resize(copies, boxes, S),
             'mkd_crop_frame   (rolled frames)': lambda: photo.crop_frames(copies, frames, S),
             'mkd_crop_frame   (the boxes as frames)': lambda: photo.crop_frames(copies, [photo.frame_from_box(b) for b in boxes], S)})
say(f'    rolled frame / box (medians): {r["mkd_crop_frame   (rolled frames)"] / r["mkd_crop_resize  (boxes)"]:.2f}')

s01 = torch.rand((len(frames), 3, S, S), generator=g).cuda()
t = (torch.rand((len(frames), 3, S, S), generator=g) * 2.0 - 1.0).cuda()
wts = torch.rand((len(frames), PS, PS), generator=g).cuda()
say(f'paste: mkd_paste_frame against mkd_paste_photo / mkd_paste_photo_weighted (1 launch each), feather {RHO}, weights {len(frames)} x {PS}^2')
r = compare({'mkd_paste_photo           (boxes)': lambda: photo.paste_photos(copies, boxes, t, s01, RHO),
             'mkd_paste_frame           (rolled frames)': lambda: photo.paste_frames(copies, frames, t, s01, RHO),
             'mkd_paste_photo_weighted  (boxes)': lambda: photo.paste_photos(copies, boxes, t, s01, RHO, weights=wts),
             'mkd_paste_frame, weights  (rolled frames)': lambda: photo.paste_frames(copies, frames, t, s01, RHO, weights=wts)})
say(f'    rolled frame / box (medians): plain {r["mkd_paste_frame           (rolled frames)"] / r["mkd_paste_photo           (boxes)"]:.2f}, '
    f'weighted {r["mkd_paste_frame, weights  (rolled frames)"] / r["mkd_paste_photo_weighted  (boxes)"]:.2f}')

say(f'frames: mkd_face_frames (4 launches) next to mkd_label_components (4 launches), one {PS}^2 map')
for K in (4, components.MAX_OUT):
    tab, _, idk = components.label_components(labels, fp.FACE_CLASSES, min_area=(PS // 32) ** 2, max_out=K, want_ids=True)
    out = torch.empty((1, K, 6), device='cuda', dtype=torch.int64)
    scratch = torch.empty((int(lib.mkd_face_frames_scratch_bytes(1, K)) + 256,), device='cuda', dtype=torch.uint8)
    sbase = (scratch.data_ptr() + 255) & ~255
    cc = torch.empty((int(lib.mkd_label_components_scratch_bytes(1, PS, PS)) + 256,), device='cuda', dtype=torch.uint8)
    cbase = (cc.data_ptr() + 255) & ~255
    tab2, cnt2, ids2 = torch.empty_like(tab), torch.empty((1,), device='cuda', dtype=torch.int32), torch.empty_like(idk)
    hw = (C.c_int32 * 2)(H, W)
    bits = components.class_bits(fp.FACE_CLASSES)
    compare({f'mkd_label_components  max_out {K:2d}': lambda: mlib.check(lib.mkd_label_components(P(labels), 1, PS, PS, C.c_uint64(bits), (PS // 32) ** 2, K, P(tab2),
                                                                                              P(cnt2), P(ids2), C.c_void_p(cbase), stream()), 'mkd_label_components'),
             f'mkd_face_frames       max_out {K:2d}': lambda: mlib.check(lib.mkd_face_frames(P(labels), P(idk), P(tab), 1, PS, K, hw, C.c_uint64(1 << 4), C.c_uint64(1 << 5),
                                                                                         max(1, (PS // 128) ** 2), P(out), C.c_void_p(sbase), stream()), 'mkd_face_frames')})
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
