"""Builds makeupdiffuse_amd/libmkd.so (gfx950 only) with hipcc. In-tree, incremental.

    python -m makeupdiffuse_amd.build [--force]
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(HERE, 'csrc', '_obj')
LIB = os.path.join(HERE, 'libmkd.so')
SOURCES = ['kernels_gemm.hip', 'kernels_conv.hip', 'kernels_norm.hip', 'kernels_attn.hip', 'kernels_tfm.hip', 'kernels_misc.hip', 'kernels_hist.hip', 'kernels_region.hip', 'kernels_photo.hip', 'kernels_video.hip', 'kernels_motion.hip', 'kernels_align.hip', 'kernels_components.hip', 'kernels_parser.hip', 'kernels_noise.hip', 'kernels_teacher.hip', 'kernels_teacher_warp.hip', 'kernels_teacher_points.hip', 'parser.hip', 'engine.hip', 'api_kernels.hip']
HEADERS = ['mkd_common.h', 'gemm_device.h', 'parser.h', 'tfm_fold.h', 'paste_guided.h', 'pgt_regions.h', 'gemm_tiles.inc', 'gemm_tuned.inc', os.path.join('..', '..', 'include', 'mkd.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function', '-Wno-unused-value', '-Wno-unused-result',
         '-ffp-contract=fast']
# mkd_pgt_warp's definition (and mkd_tps_solve's) rounds every double operation on its own.  Under -ffp-contract=fast the backend fuses a product into a
# following sum whatever `#pragma clang fp contract(off)` says in the source, so these translation units turn contraction off as a whole
# (the last flag wins); the fused operations inside the device's log and division stay, they are explicit.
SOURCE_FLAGS = {'kernels_teacher_warp.hip': ['-ffp-contract=off'], 'kernels_teacher_points.hip': ['-ffp-contract=off']}


def _hipcc() -> str:
    for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if c and os.path.exists(c):
            return c
    raise RuntimeError('hipcc not found: libmkd.so cannot be built (there is no CPU fallback)')


def _digest(paths, flags) -> str:
    h = hashlib.sha256()
    for p in paths:
        with open(p, 'rb') as f:
            h.update(f.read())
    h.update(' '.join(flags).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS]
    objs, jobs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        op = os.path.join(OBJ, src + '.o')
        stamp = op + '.sha'
        flags = FLAGS + SOURCE_FLAGS.get(src, [])
        dg = _digest([sp] + hdrs, flags)
        old = open(stamp).read() if os.path.exists(stamp) else ''
        if force or not os.path.exists(op) or old != dg:
            cmd = [hipcc] + flags + ['-c', sp, '-o', op]
            if verbose:
                print('[mkd build]', ' '.join(cmd), flush=True)
            jobs.append((subprocess.Popen(cmd), cmd, stamp, dg))          # translation units compile concurrently (21 of them)
        objs.append(op)
    rebuilt = bool(jobs)
    failed = None
    for proc, cmd, stamp, dg in jobs:
        if proc.wait() != 0:
            failed = failed or cmd
        else:
            with open(stamp, 'w') as f:
                f.write(dg)
    if failed:
        raise subprocess.CalledProcessError(1, failed)
    if rebuilt or not os.path.exists(LIB):
        cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
        if verbose:
            print('[mkd build]', ' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
