#!/usr/bin/env python
"""CPU only: writes tests/golden/hist_match_ref.npz from the REFERENCE's own functions.

    python tools/make_hist_golden.py --reference <checkout of jiean001/MakeupDiffuse> [--out tests/golden/hist_match_ref.npz]

The reference's diffmk/histogram_matching.py is loaded by path (its last line calls .cuda(): torch.Tensor.cuda is the identity for
this run, and .cpu() copies as it does from a device tensor) and diffmk/makeups.py is imported behind stub modules for the packages that are not vendored (cldm.cldm with a dummy
ControlLDM, ldm.models.diffusion.ddim, diffmk.utils, diffmk.cddim); the region masks and the criterionHis values come from the
reference's own methods bound to a bare namespace object.  The fixture holds inputs and recorded results only:

  per case k (two synthetic face layouts A / B and one image on each; SR = A, R = B, RS = B, S = A):
    c{k}_img_a, c{k}_img_b   uint16 [3,H,W]   x = q / 65535 (so int(v) truncation is exercised)
    c{k}_seg_a, c{k}_seg_b   uint8  [H,W]     label maps
    c{k}_mask_a, c{k}_mask_b uint8  [4,H,W]   lip, skin, eye_left, eye_right;  c{k}_count_a / _b  int32 [4]
    c{k}_tables uint8 [8,3,256], c{k}_matched uint8 [8,3,H,W], c{k}_loss float32 [8]
        term 2 r + d: region r, d = 0: A matched to B under (mask_a, mask_b); d = 1: B matched to A under (mask_b, mask_a)
  provenance: JSON, which reference function produced each array."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS = ('lip', 'skin', 'eye_left', 'eye_right')


def load_reference(ref_root: str):
    """-> (histogram_matching module, makeups.BaseModel class) of the reference checkout"""
    torch.Tensor.cuda = lambda self, *a, **k: self
    # on the reference's device .cpu() is a copy; on a CPU tensor it would alias, histogram_matching would then write the matched
    # values INTO criterionHis' own operand and every loss would read 0
    torch.Tensor.cpu = lambda self, *a, **k: self.clone()
    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    saved = {k: sys.modules.get(k) for k in ('diffmk', 'diffmk.histogram_matching', 'diffmk.cddim', 'diffmk.utils', 'cldm', 'cldm.cldm',
                                             'ldm', 'ldm.models', 'ldm.models.diffusion', 'ldm.models.diffusion.ddim')}
    pkg = types.ModuleType('diffmk'); pkg.__path__ = []
    sys.modules['diffmk'] = pkg
    hm = by_path('diffmk.histogram_matching', os.path.join(ref_root, 'diffmk', 'histogram_matching.py'))
    cldm = types.ModuleType('cldm.cldm'); cldm.ControlLDM = type('ControlLDM', (), {})
    cldm.__all__ = ['ControlLDM']
    stubs = {'cldm': types.ModuleType('cldm'), 'cldm.cldm': cldm, 'diffmk.cddim': types.ModuleType('diffmk.cddim'),
             'diffmk.utils': types.ModuleType('diffmk.utils'), 'ldm': types.ModuleType('ldm'), 'ldm.models': types.ModuleType('ldm.models'),
             'ldm.models.diffusion': types.ModuleType('ldm.models.diffusion'),
             'ldm.models.diffusion.ddim': types.ModuleType('ldm.models.diffusion.ddim')}
    stubs['diffmk.cddim'].MKDDIMSampler = object
    stubs['diffmk.utils'].get_grid_image = None
    stubs['ldm.models.diffusion.ddim'].DDIMSampler = object
    sys.modules.update(stubs)
    mk = by_path('_reference_makeups', os.path.join(ref_root, 'diffmk', 'makeups.py'))
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v
    return hm, mk.BaseModel


# ---- synthetic inputs ------------------------------------------------------------------------------------------------------------
def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def face_layout(H, W, cy, cx, ry, rx, eye_dy, eye_dx, eye_r, lip_dy, lip_r, nose=True):
    """labels: 0 background, 1 face skin, 4 / 5 eyes, 6 nose, 7 / 9 lips, 12 hair, 13 neck (fractions of H, W)"""
    seg = np.zeros((H, W), np.uint8)
    seg[ellipse(H, W, (cy + ry * 0.95) * H, cx * W, 0.18 * H, rx * 0.55 * W)] = 13
    seg[ellipse(H, W, (cy - ry * 0.55) * H, cx * W, ry * 0.75 * H, rx * 1.1 * W)] = 12
    seg[ellipse(H, W, cy * H, cx * W, ry * H, rx * W)] = 1
    if nose:
        seg[ellipse(H, W, (cy + 0.02) * H, cx * W, 0.07 * H, 0.03 * W)] = 6
    seg[ellipse(H, W, (cy - eye_dy) * H, (cx - eye_dx) * W, eye_r[0] * H, eye_r[1] * W)] = 4
    seg[ellipse(H, W, (cy - eye_dy) * H, (cx + eye_dx) * W, eye_r[0] * H, eye_r[1] * W)] = 5
    up = ellipse(H, W, (cy + lip_dy) * H, cx * W, lip_r[0] * H, lip_r[1] * W)
    seg[up] = 7
    seg[up & (np.mgrid[0:H, 0:W][0] > (cy + lip_dy) * H)] = 9
    return seg


def field(H, W, seed, block=2):
    """[3,H,W] in [0,1]: a smooth ramp plus noise, constant on block x block pixels (keeps the compressed fixture small)"""
    g = np.random.default_rng(seed)
    h, w = (H + block - 1) // block, (W + block - 1) // block
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for c in range(3):
        u = 0.5 + 0.35 * np.sin(yy / h * (2.0 + c) + 0.7 * c) * np.cos(xx / w * (3.0 - 0.5 * c)) + 0.15 * g.standard_normal((h, w))
        out.append(np.kron(np.clip(u, 0, 1), np.ones((block, block)))[:H, :W])
    return np.stack(out)


def quant(x):
    return np.round(np.clip(x, 0, 1) * 65535.0).astype(np.uint16)


def make_cases():
    cases = []
    # 0: 128^2, dst tone x^2 against 0.3 + 0.6 x
    sa = face_layout(128, 128, 0.52, 0.50, 0.34, 0.27, 0.10, 0.11, (0.025, 0.05), 0.19, (0.035, 0.09))
    sb = face_layout(128, 128, 0.50, 0.53, 0.31, 0.25, 0.09, 0.10, (0.03, 0.045), 0.17, (0.03, 0.08))
    cases.append((quant(field(128, 128, 11) ** 2), quant(0.3 + 0.6 * field(128, 128, 12)), sa, sb))
    # 1: 128^2, another layout; B's lips are ONE value (a single-spike histogram), A is dark / gamma 0.5
    sa = face_layout(128, 128, 0.48, 0.47, 0.30, 0.24, 0.08, 0.10, (0.03, 0.05), 0.16, (0.04, 0.07), nose=False)
    sb = face_layout(128, 128, 0.55, 0.50, 0.33, 0.28, 0.11, 0.12, (0.025, 0.055), 0.20, (0.03, 0.10))
    a = quant(0.05 + 0.9 * np.sqrt(field(128, 128, 21)))
    b = quant(0.6 * field(128, 128, 22) ** 2)
    lips = np.isin(sb, (7, 9))
    for c, val in enumerate((47001, 9000, 13333)):
        b[c][lips] = val
    cases.append((a, b, sa, sb))
    # 2: 256^2 with a >= 15000-pixel skin region
    sa = face_layout(256, 256, 0.50, 0.50, 0.36, 0.29, 0.10, 0.11, (0.025, 0.05), 0.20, (0.035, 0.09))
    sb = face_layout(256, 256, 0.52, 0.48, 0.35, 0.28, 0.09, 0.12, (0.03, 0.05), 0.18, (0.03, 0.08))
    cases.append((quant(field(256, 256, 31, 4) ** 2), quant(0.3 + 0.6 * field(256, 256, 32, 4)), sa, sb))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a reference checkout (holds diffmk/histogram_matching.py, diffmk/makeups.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'hist_match_ref.npz'))
    args = ap.parse_args()
    hm, BaseModel = load_reference(args.reference)
    ns = types.SimpleNamespace(criterionL1=torch.nn.L1Loss())
    for name in ('get_msk_lip', 'get_msk_skin', 'get_msk_eye', 'mask_preprocess', 'rebound_box', 'criterionHis'):
        setattr(ns, name, types.MethodType(getattr(BaseModel, name), ns))

    out, timing = {}, {}
    for k, (qa, qb, sa, sb) in enumerate(make_cases()):
        H, W = sa.shape
        for s in (sa, sb):          # goldens keep the eyes >= 10 px from the border (the reference's negative slice start wraps)
            for lab in (4, 5):
                ys, xs = np.nonzero(s == lab)
                assert ys.min() >= 10 and xs.min() >= 10 and ys.max() < H - 10 and xs.max() < W - 10, 'eye too close to the border'
        A = torch.from_numpy(qa.astype(np.float32) / np.float32(65535.0))[None]
        B = torch.from_numpy(qb.astype(np.float32) / np.float32(65535.0))[None]
        la, lb = torch.from_numpy(sa.astype(np.float32))[None, None], torch.from_numpy(sb.astype(np.float32))[None, None]
        lip = ns.get_msk_lip(la, lb)
        skin = ns.get_msk_skin(la, lb)
        eye = ns.get_msk_eye(la.clone(), lb.clone())
        regions = {'lip': lip, 'skin': skin, 'eye_left': eye[0:4], 'eye_right': eye[4:8]}
        mask_a = np.stack([regions[r][0][0, 0].numpy() for r in REGIONS])
        mask_b = np.stack([regions[r][1][0, 0].numpy() for r in REGIONS])
        assert set(np.unique(mask_a)) <= {0.0, 1.0} and set(np.unique(mask_b)) <= {0.0, 1.0}
        tables = np.zeros((8, 3, 256), np.uint8)
        matched = np.zeros((8, 3, H, W), np.uint8)
        loss = np.zeros(8, np.float32)
        t0 = time.perf_counter()
        for r, name in enumerate(REGIONS):
            mA, mB, idxA, idxB = regions[name]
            for d, (dst, ref, md, mr, idx) in enumerate(((A, B, mA, mB, idxA), (B, A, mB, mA, idxB))):
                t = 2 * r + d
                loss[t] = float(ns.criterionHis(dst, ref, md, mr, idx))
                # what criterionHis hands to histogram_matching, and the two functions that one calls
                din = (dst * 255).squeeze() * md.expand(1, 3, H, W).squeeze()
                rin = (ref * 255).squeeze() * mr.expand(1, 3, H, W).squeeze()
                m = hm.histogram_matching(din, rin, idx).numpy()
                assert np.array_equal(m, np.round(m)) and m.min() >= 0 and m.max() <= 255
                matched[t] = m.astype(np.uint8)
                ix = [x.numpy() for x in idx]
                dn, rn = din.numpy(), rin.numpy()
                hd = hm.cal_hist([dn[c, ix[0], ix[1]] for c in range(3)])
                hr = hm.cal_hist([rn[c, ix[2], ix[3]] for c in range(3)])
                tables[t] = np.array([hm.cal_trans(hd[c], hr[c]) for c in range(3)], dtype=np.uint8)
        timing[f'c{k}'] = time.perf_counter() - t0
        out.update({f'c{k}_img_a': qa, f'c{k}_img_b': qb, f'c{k}_seg_a': sa, f'c{k}_seg_b': sb,
                    f'c{k}_mask_a': mask_a.astype(np.uint8), f'c{k}_mask_b': mask_b.astype(np.uint8),
                    f'c{k}_count_a': mask_a.reshape(4, -1).sum(1).astype(np.int32), f'c{k}_count_b': mask_b.reshape(4, -1).sum(1).astype(np.int32),
                    f'c{k}_tables': tables, f'c{k}_matched': matched, f'c{k}_loss': loss})
        print(f'case {k}: {H}x{W} counts A {out[f"c{k}_count_a"].tolist()} B {out[f"c{k}_count_b"].tolist()} '
              f'reference time {timing[f"c{k}"]:.2f} s for 8 terms, loss {loss.tolist()}')
    prov = {'c*_img_*, c*_seg_*': 'synthetic inputs drawn by tools/make_hist_golden.py (no reference function)',
            'c*_mask_*': 'reference diffmk/makeups.py BaseModel.get_msk_lip / get_msk_skin / get_msk_eye (bound to a bare namespace)',
            'c*_count_*': 'pixel sums of the c*_mask_* arrays (the reference keeps index lists, not counts)',
            'c*_loss': 'reference diffmk/makeups.py BaseModel.criterionHis (torch.nn.L1Loss, fp32)',
            'c*_matched': 'reference diffmk/histogram_matching.py histogram_matching on the operands criterionHis builds',
            'c*_tables': 'reference diffmk/histogram_matching.py cal_trans(cal_hist(dst), cal_hist(ref)) on the same operands',
            'restatement': 'none of the arrays comes from the restatement (tests/hist_match_ref.py)'}
    out['provenance'] = np.array(json.dumps(prov))
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
