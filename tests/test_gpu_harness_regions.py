"""runs/test.py --region-refs end to end on the device, in a fresh child process: pair folder + scgan_segs label maps -> the usual
passes -> TestDiffuseModel.transfer_regions -> the samples_regions grid."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_runs_test_py_writes_the_samples_regions_grid(tmp_path):
    import torch
    from PIL import Image
    data = tmp_path / 'data'
    rng = np.random.default_rng(5)
    seg = np.zeros((64, 64), np.uint8)                       # skin with two eyes and lips, as the face parser labels them
    seg[8:56, 12:52] = 1; seg[20:24, 18:26] = 4; seg[20:24, 38:46] = 5; seg[40:43, 24:40] = 7; seg[43:46, 24:40] = 9
    for d, n in (('non-makeup', 's1.png'), ('makeup', 'r1.png'), ('makeup', 'lip.png'), ('makeup', 'eye.png')):
        os.makedirs(data / 'images' / d, exist_ok=True); os.makedirs(data / 'scgan_segs' / d, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(data / 'images' / d / n)
        Image.fromarray(seg, mode='L').save(data / 'scgan_segs' / d / n)
    (data / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--data-root', str(data), '--res', '64', '--batch-size', '1',
                        '--ddim-steps', '2', '--seed', '7', '--out', str(out), '--region-refs', 'lip=makeup/lip.png,eye=makeup/eye.png',
                        '--region-strength', 'lip=0.7', '--region-feather', '1'],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png',
                     'samples_regions_0000.png'], names
    g = np.asarray(Image.open(root / 'samples_regions_0000.png'))
    assert g.ndim == 3 and g.shape[2] == 3 and g.dtype == np.uint8 and g.std() > 1.0           # a decoded image, not a constant
    lat = torch.load(out / 'latents_0000.pt', weights_only=True)
    assert tuple(lat['samples_regions_latent'].shape) == (1, 4, 8, 8) and torch.isfinite(lat['samples_regions_latent']).all()
    assert not torch.equal(lat['samples_regions_latent'], lat['samples_latent'])               # the two references act
