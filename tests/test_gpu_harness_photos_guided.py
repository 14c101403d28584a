"""runs/test.py --photos --guided-paste end to end on the device, in a fresh child process (the layout of
tests/test_gpu_harness_photos.py): the photo comes back at its own size with every byte outside the box kept and the box made up, the
run says which guide it used, and the guide's options are refused without --guided-paste or out of range."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(tmp_path / 'data'), '--res', '64', '--batch-size', '1',
                           '--ddim-steps', '2', '--seed', '7', '--out', str(tmp_path / 'out'), *extra], capture_output=True, text=True, timeout=900,
                          cwd=str(tmp_path))


def test_runs_test_py_pastes_guided(tmp_path):
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(16)
    photos = {'non-makeup/s1.png': rng.integers(0, 256, (90, 120, 3), dtype=np.uint8), 'makeup/r1.png': rng.integers(0, 256, (70, 50, 3), dtype=np.uint8)}
    for name, arr in photos.items():
        os.makedirs(data / 'images' / os.path.dirname(name), exist_ok=True)
        Image.fromarray(arr).save(data / 'images' / name)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    (data / 'boxes.txt').write_text('non-makeup/s1.png 20 5 72 70\n')
    # refused before any model is built: the guide's options without the switch, a radius out of range
    for extra, word in ((('--photos', '--guide-radius', '2'), '--guided-paste'), (('--photos', '--guided-paste', '--guide-radius', '3'), 'radius')):
        r = run(tmp_path, *extra)
        assert r.returncode != 0 and word in r.stderr and not os.path.exists(tmp_path / 'out' / 'photos'), (extra, r.stderr[-2000:])
    r = run(tmp_path, '--photos', '--photo-feather', '2', '--guided-paste', '--guide-radius', '2', '--guide-sigma', '12.5')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'guided paste: radius 2, sigma 12.5' in r.stdout
    out = tmp_path / 'out'
    assert sorted(os.listdir(out / 'photos')) == ['s1&r1.png']
    got = np.asarray(Image.open(out / 'photos' / 's1&r1.png'))
    src = photos['non-makeup/s1.png']
    assert got.shape == src.shape and got.dtype == np.uint8
    inside = np.zeros(src.shape[:2], bool)
    inside[5:75, 20:92] = True
    assert np.array_equal(got[~inside], src[~inside]), f'{int((got[~inside] != src[~inside]).sum())} bytes outside the box changed'
    assert (got[inside] != src[inside]).mean() > 0.3, 'the face box is the source too'
