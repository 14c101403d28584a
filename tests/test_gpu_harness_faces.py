"""runs/test.py --photos --max-faces end to end on the device, in a fresh child process: photos of their own sizes, the faces from a
(randomly initialised) face parser -- whatever components its label maps hold are found on the device -- or from a boxes file with one
line per face; every face is sampled and pasted back -> one PNG per pair with the source photo's size."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('faces_from', ['parser', 'boxes'])
def test_runs_test_py_group_photos(tmp_path, faces_from):
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(26)
    photos = {'non-makeup/s1.png': rng.integers(0, 256, (90, 120, 3), dtype=np.uint8), 'makeup/r1.png': rng.integers(0, 256, (70, 50, 3), dtype=np.uint8)}
    for name, arr in photos.items():
        os.makedirs(data / 'images' / os.path.dirname(name), exist_ok=True)
        Image.fromarray(arr).save(data / 'images' / name)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    boxes = [(5, 8, 50, 50), (70, 30, 40, 40), (0, 0, 20, 20)]                      # three lines for the source: --max-faces 2 takes the first two
    if faces_from == 'boxes':
        (data / 'boxes.txt').write_text(''.join('non-makeup/s1.png %d %d %d %d\n' % b for b in boxes))
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(data), '--res', '64', '--batch-size', '1',
                        '--ddim-steps', '2', '--seed', '7', '--out', str(out), '--photos', '--max-faces', '2'] +
                       (['--face-parser', 'random'] if faces_from == 'parser' else []),
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'faces per photo: [' in r.stdout
    assert sorted(os.listdir(out / 'photos')) == ['s1&r1.png']
    got = np.asarray(Image.open(out / 'photos' / 's1&r1.png'))
    src = photos['non-makeup/s1.png']
    assert got.shape == src.shape and got.dtype == np.uint8
    if faces_from == 'boxes':
        assert 'faces per photo: [2]' in r.stdout
        inside = np.zeros(src.shape[:2], bool)
        for x0, y0, bw, bh in boxes[:2]:
            inside[y0:y0 + bh, x0:x0 + bw] = True
            assert (got[y0:y0 + bh, x0:x0 + bw] != src[y0:y0 + bh, x0:x0 + bw]).mean() > 0.3, 'a face box is the source too'
        assert np.array_equal(got[~inside], src[~inside]), f'{int((got[~inside] != src[~inside]).sum())} bytes outside the two boxes changed'
    names = sorted(os.listdir(out / 'makeupdiffuse_mi355x'))                       # the usual passes are untouched
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
