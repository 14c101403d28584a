#!/usr/bin/env python
"""CPU only: writes tests/golden/photo_resize.npz from Pillow's own resize, so that no test needs Pillow to check mkd_crop_resize.

    python tools/make_photo_golden.py [--out tests/golden/photo_resize.npz]

The fixture holds inputs and recorded results only:
  photo{i}        uint8 [H,W,3]   synthetic photos (noise on 2 x 2 blocks over a ramp, plain noise, a 0 / 255 image, a wide strip)
  cases           JSON list of {photo, box: [x0, y0, w, h], size}
  out{k}          uint8 [S,S,3]   np.asarray(Image.fromarray(photo).resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + w, y0 + h)))
  pillow          the Pillow version that wrote it"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (photo, (x0, y0, w, h), size)
CASES = [
    (0, (20, 10, 122, 122), 37),        # shrinks x 3.3: 9 taps
    (0, (50, 60, 9, 11), 16),           # enlarges
    (0, (0, 0, 100, 90), 16),           # flush with the left and top edge, not square
    (0, (123, 80, 80, 70), 37),         # flush with the right and bottom edge
    (2, (0, 0, 64, 64), 64),            # the whole photo, W = S
    (1, (5, 10, 50, 80), 64),           # enlarges in x, shrinks in y
    (1, (0, 0, 64, 97), 16),            # a whole non-square photo
    (3, (3, 2, 190, 36), 37),           # shrinks x 5.1 in x, enlarges in y
    (2, (7, 9, 41, 33), 16),            # 0 / 255 pixels
    (0, (0, 30, 203, 100), 64),         # flush left and right
    (0, (60, 0, 75, 150), 16),          # flush top and bottom, 21 taps in y
    (0, (10, 20, 64, 64), 64),          # scale 1, integer box: Pillow skips both passes
]


def make_photos():
    g = np.random.default_rng(20261018)
    yy, xx = np.mgrid[0:150, 0:203]
    ramp = (yy * 0.9 + xx * 0.6)[..., None] + np.array([0.0, 40.0, 90.0])
    noise = np.kron(g.integers(-70, 71, (75, 102, 3)), np.ones((2, 2, 1)))[:150, :203]
    p0 = np.clip(ramp + noise, 0, 255).astype(np.uint8)
    p1 = g.integers(0, 256, (97, 64, 3), dtype=np.uint8)
    p2 = (g.integers(0, 2, (64, 64, 3)) * 255).astype(np.uint8)
    p3 = np.kron(g.integers(0, 256, (20, 100, 3)), np.ones((2, 2, 1))).astype(np.uint8)
    return [p0, p1, p2, p3]


def main():
    from PIL import Image
    import PIL
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'photo_resize.npz'))
    args = ap.parse_args()
    photos = make_photos()
    out = {f'photo{i}': p for i, p in enumerate(photos)}
    cases = []
    for k, (pi, (x0, y0, bw, bh), S) in enumerate(CASES):
        H, W = photos[pi].shape[:2]
        assert 0 <= x0 and 0 <= y0 and x0 + bw <= W and y0 + bh <= H
        img = Image.fromarray(photos[pi]).resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + bw, y0 + bh))
        out[f'out{k}'] = np.asarray(img, dtype=np.uint8)
        cases.append({'photo': pi, 'box': [x0, y0, bw, bh], 'size': S})
    out['cases'] = np.array(json.dumps(cases))
    out['pillow'] = np.array(PIL.__version__)
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes, {len(cases)} cases, Pillow {PIL.__version__}')


if __name__ == '__main__':
    main()
