"""runs/test.py --photos end to end on the device, in a fresh child process: a pair folder with photos of different sizes and a
boxes.txt -> the usual passes, then <out>/photos/<pair>.png at the source photo's own size with every byte outside the box kept."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_runs_test_py_writes_the_source_photo_with_the_face_box_replaced(tmp_path):
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(16)
    photos = {'non-makeup/s1.png': rng.integers(0, 256, (90, 120, 3), dtype=np.uint8), 'makeup/r1.png': rng.integers(0, 256, (70, 50, 3), dtype=np.uint8)}
    for name, arr in photos.items():
        os.makedirs(data / 'images' / os.path.dirname(name), exist_ok=True)
        Image.fromarray(arr).save(data / 'images' / name)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    (data / 'boxes.txt').write_text('non-makeup/s1.png 20 5 72 70\n')             # the reference photo takes the centred largest square
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(data), '--res', '64', '--batch-size', '1',
                        '--ddim-steps', '2', '--seed', '7', '--out', str(out), '--photos', '--photo-feather', '2'],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out / 'photos')) == ['s1&r1.png']
    got = np.asarray(Image.open(out / 'photos' / 's1&r1.png'))
    src = photos['non-makeup/s1.png']
    assert got.shape == src.shape and got.dtype == np.uint8
    inside = np.zeros(src.shape[:2], bool)
    inside[5:75, 20:92] = True
    assert np.array_equal(got[~inside], src[~inside]), f'{int((got[~inside] != src[~inside]).sum())} bytes outside the box changed'
    assert (got[inside] != src[inside]).mean() > 0.3, 'the face box is the source too'
    names = sorted(os.listdir(out / 'makeupdiffuse_mi355x'))                       # the usual passes are untouched
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
