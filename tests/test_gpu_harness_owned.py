"""runs/test.py --photos --max-faces 2 --own-pixels end to end on the device, in a fresh child process: the faces and their owner map
come from a (randomly initialised) face parser -- whatever components its label maps hold -- and every face is pasted onto its own
pixels -> one PNG per pair with the source photo's size."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_runs_test_py_group_photos_own_pixels(tmp_path):
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(27)
    photos = {'non-makeup/s1.png': rng.integers(0, 256, (90, 120, 3), dtype=np.uint8), 'makeup/r1.png': rng.integers(0, 256, (70, 50, 3), dtype=np.uint8)}
    for name, arr in photos.items():
        os.makedirs(data / 'images' / os.path.dirname(name), exist_ok=True)
        Image.fromarray(arr).save(data / 'images' / name)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(data), '--res', '64', '--batch-size', '1',
                        '--ddim-steps', '2', '--seed', '7', '--out', str(out), '--photos', '--max-faces', '2', '--own-pixels', '--own-feather', '1',
                        '--face-parser', 'random'], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'faces per photo: [' in r.stdout
    assert sorted(os.listdir(out / 'photos')) == ['s1&r1.png']
    got = np.asarray(Image.open(out / 'photos' / 's1&r1.png'))
    src = photos['non-makeup/s1.png']
    assert got.shape == src.shape and got.dtype == np.uint8
    names = sorted(os.listdir(out / 'makeupdiffuse_mi355x'))                       # the usual passes are untouched
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
