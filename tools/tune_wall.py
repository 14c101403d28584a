#!/usr/bin/env python
"""Whole-loop GEMM tuner (run on the GPU box): coordinate descent on the WALL time of the captured sampling loop.

tools/tune_gemm.py (each shape alone) and tools/tune_ineval.py (per-launch times of a serial evaluation) both minimise a kernel's own
duration.  The sampling loop runs two chains of ~400 dependent launches concurrently, and there a kernel's duration is not what it
costs: a tile choice that is 10 % slower alone can be free (it runs beside the other chain) or one that is faster alone can cost
(it takes the CUs the other chain's latency-critical kernels need).  So this tuner changes ONE shape's (tile config, split-K),
re-plans, replays the hipGraph loop and keeps the change only when the loop itself got faster, twice.

    python tools/tune_wall.py --batch 8 --res 256 --out gpurun_out/wall_b8_r256.json
"""
import argparse
import collections
import csv
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from makeupdiffuse_amd import lib as mlib  # noqa: E402
from makeupdiffuse_amd.engine import MkdEngine, NetConfig  # noqa: E402
from makeupdiffuse_amd.schedule import DDIMSchedule  # noqa: E402

TILE_M, TILE_N, PATCH, _ = zip(*mlib.tile_table())      # the library's tile table, by configuration index (needs no GPU)
KEYS = ('M', 'N', 'K', 'conv', 'stride', 'up', 'Hin', 'Win', 'Cin', 'Hout', 'Wout', 'splitk')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--min-us', type=float, default=40.0, help='only shapes with at least this much serial time per evaluation')
    ap.add_argument('--gain', type=float, default=0.003, help='relative wall-time gain a change must show (twice) to be kept')
    ap.add_argument('--budget-s', type=float, default=600.0)
    ap.add_argument('--interp', type=int, default=0, help='makeup interpolation sweep: --batch sources x this many alpha points (BASELINE config 5)')
    ap.add_argument('--cfgs', default=None, help='comma list: only these tile configurations are candidates')
    ap.add_argument('--skip', type=int, default=0, help='start at this shape (shapes are ordered by their serial time)')
    ap.add_argument('--out', default='gpurun_out/wall.json')
    args = ap.parse_args()
    lib = mlib.load()
    eng = MkdEngine(NetConfig()); eng.init_random(0)
    g = torch.Generator().manual_seed(0)
    h = args.res // 8
    nb = args.batch * max(1, args.interp)
    hint = torch.rand(nb, 6, args.res, args.res, generator=g).cuda()
    ctx = torch.randn(nb, 77, 768, generator=g).cuda()
    x = torch.randn(nb, 4, h, h, generator=g).cuda()
    t = torch.full((nb,), 500).cuda()
    hint2 = torch.rand(nb, 6, args.res, args.res, generator=g).cuda() if args.interp else None
    alpha = torch.linspace(0.0, 1.0, args.interp).repeat(args.batch).cuda() if args.interp else None
    sch = DDIMSchedule().make_ddim(args.steps)

    def wall(reps=args.reps):
        eng.prepare(hint, ctx, hint2=hint2, alpha=alpha) if args.interp else eng.prepare(hint, ctx)
        best = 1e9
        for _ in range(reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            eng.sample(x, sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas, use_graph=True)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3 / args.steps)
        return best

    lib.mkd_gemm_set_override(0, 0, 0, 0, 0, 0, -1, 0)
    eng.prepare(hint, ctx, hint2=hint2, alpha=alpha) if args.interp else eng.prepare(hint, ctx)
    eng.eps_profile(x, t, csv_path='/tmp/wall_ops.csv')
    shapes = collections.OrderedDict()
    for r in csv.DictReader(open('/tmp/wall_ops.csv')):
        if not r['kind'].startswith('gemm_'):
            continue
        kv = dict(re.findall(r'(\w+)=(-?\d+)', r['label']))
        key = tuple(int(kv[k]) for k in KEYS)
        n, us = shapes.get(key, (0, 0.0))
        shapes[key] = (n + 1, us + float(r['ms']) * 1e3)
    order = [k for k in sorted(shapes, key=lambda k: -shapes[k][1]) if shapes[k][1] >= args.min_us]
    cur = wall(5)
    print(f'{len(shapes)} GEMM shapes, {len(order)} with >= {args.min_us} us per evaluation; wall {cur:.4f} ms/eval', flush=True)
    t_start = time.time()
    kept = {}
    only = [int(c) for c in args.cfgs.split(',')] if args.cfgs else None
    for si, sh in enumerate(order):
        if si < args.skip:
            continue
        if time.time() - t_start > args.budget_s:
            print('time budget reached', flush=True)
            break
        M, N, K, conv, stride, up, Hin, Win, Cin, Hout, Wout, sk = sh
        cands = []
        for cfg in (only if only else range(len(TILE_M))):
            if not lib.mkd_gemm_cfg_supported(cfg, M, N, K, conv, Hin, Win, Cin, Hout, Wout, stride, up):
                continue
            patch = PATCH[cfg]
            if patch and not (conv and stride == 1 and up == 0 and Cin % 64 == 0):
                continue
            tiles = -(-M // TILE_M[cfg]) * -(-N // TILE_N[cfg])
            units = Cin // 64 if patch else (K + 63) // 64
            ss = {1, sk}
            for want in (128, 256, 512):
                ss.add(max(1, min(units // (1 if patch else 2), -(-want // tiles), 24)))
            for s in sorted(ss):
                if s > 1 and (tiles * s > 2048 or s * M * N * 4 > (256 << 20)):
                    continue
                if 48 <= tiles * s:
                    cands.append((cfg, s))
        best = None
        for cfg, s in cands:
            lib.mkd_gemm_set_override(M, N, K, conv, stride, up, cfg, s)
            w = wall()
            if best is None or w < best[0]:
                best = (w, cfg, s)
        if best and best[0] < cur * (1 - args.gain):
            lib.mkd_gemm_set_override(M, N, K, conv, stride, up, best[1], best[2])
            w2 = wall(5)                                   # must hold up on a second, longer measurement
            if w2 < cur * (1 - args.gain):
                kept['_'.join(map(str, sh[:6]))] = {'shape': list(sh[:11]), 'count': shapes[sh][0], 'best_cfg': best[1], 'best_splitk': best[2],
                                                    'best_us': 0.0, 'default_us': 0.0, 'wall_ms_before': cur, 'wall_ms_after': w2}
                print(f'[{si + 1}/{len(order)}] M={M} N={N} K={K} conv={conv} s={stride} up={up} x{shapes[sh][0]}: cfg {best[1]} splitk {best[2]} '
                      f'wall {cur:.4f} -> {w2:.4f} ms/eval   ({len(cands)} candidates, {time.time() - t_start:.0f} s)', flush=True)
                cur = w2
                json.dump(kept, open(args.out, 'w'), separators=(',', ':'))
                continue
        lib.mkd_gemm_set_override(M, N, K, conv, stride, up, -1, 0)          # back to the table entry
        print(f'[{si + 1}/{len(order)}] M={M} N={N} K={K} conv={conv} x{shapes[sh][0]}: table stays (best candidate {best[0] if best else float("nan"):.4f} vs {cur:.4f})', flush=True)
    final = wall(5)
    print(f'wall {final:.4f} ms/eval with {len(kept)} shapes changed', flush=True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    json.dump(kept, open(args.out, 'w'), separators=(',', ':'))
    lib.mkd_gemm_set_override(0, 0, 0, 0, 0, 0, -1, 0)
    eng.close()


if __name__ == '__main__':
    main()
