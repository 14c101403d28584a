"""runs/test.py --teacher hist --teacher-start end to end on the device, in a fresh child process: pair folder + scgan_segs label maps
of both images -> the usual rows plus the teacher's, the teacher's score beside the samples', and a teacher image that is the source
outside the regions."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_runs_test_py_writes_the_teacher_rows(tmp_path):
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
                        '--ddim-steps', '5', '--seed', '7', '--device-noise', '--out', str(out), '--teacher', 'hist', '--teacher-feather', '0',
                        '--teacher-start', '0.6', '--makeup-score'],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'ground_truth_0000.png', 'reconstruction_0000.png', 'sample_ddmp_0000.png',
                     'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
    src = np.asarray(Image.open(root / 'control_src_0000.png'))
    gt = np.asarray(Image.open(root / 'ground_truth_0000.png'))
    assert gt.shape == src.shape == (64, 64, 3)
    region = np.isin(seg, (1, 6, 13, 7, 9))                  # feather 0: outside the lip / skin (and eye: skin labels) regions x_p is the source
    assert np.array_equal(gt[~region], src[~region]) and (gt[region] != src[region]).mean() > 0.5
    rows = [l.split(',') for l in (out / 'makeup_score.csv').read_text().splitlines()[1:]]
    entries = sorted(row[1] for row in rows)
    assert entries == ['makeup_hist', 'makeup_hist_cfg_scale_9.00', 'makeup_hist_teacher'], entries
    teacher_row = [float(v) for row in rows if row[1] == 'makeup_hist_teacher' for v in row[2:]]
    assert len(teacher_row) == 4 and all(np.isfinite(teacher_row))
