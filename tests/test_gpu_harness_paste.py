"""runs/test.py --paste-background end to end on the device, in a fresh child process: pair folder + scgan_segs label maps -> the usual
passes -> every decoded sample keeps the source's PNG bytes over background, teeth and hair."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_runs_test_py_keeps_the_source_bytes_over_the_background(tmp_path):
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(6)
    seg = np.zeros((64, 64), np.uint8)                       # background around hair, skin with two eyes, lips and teeth
    seg[2:10, 10:54] = 12; seg[10:56, 12:52] = 1; seg[20:24, 18:26] = 4; seg[20:24, 38:46] = 5
    seg[40:43, 24:40] = 7; seg[43:44, 28:36] = 11; seg[44:47, 24:40] = 9
    for d, n in (('non-makeup', 's1.png'), ('makeup', 'r1.png')):
        os.makedirs(data / 'images' / d, exist_ok=True); os.makedirs(data / 'scgan_segs' / d, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(data / 'images' / d / n)
        Image.fromarray(seg, mode='L').save(data / 'scgan_segs' / d / n)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(data), '--res', '64', '--batch-size', '1',
                        '--ddim-steps', '2', '--seed', '7', '--out', str(out), '--paste-background'],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
    src = np.asarray(Image.open(root / 'control_src_0000.png'))
    assert src.shape == (64, 64, 3) and src.dtype == np.uint8
    keep = np.isin(seg, (0, 11, 12))
    assert keep.any() and not keep.all()
    for n in ('samples_0000.png', 'samples_cfg_scale_9.00_0000.png'):
        img = np.asarray(Image.open(root / n))
        assert img.shape == src.shape and img.dtype == np.uint8
        assert np.array_equal(img[keep], src[keep]), f'{n}: {int((img[keep] != src[keep]).sum())} background bytes differ from the source'
        assert (img[~keep] != src[~keep]).mean() > 0.5, f'{n}: the face is the source too'
