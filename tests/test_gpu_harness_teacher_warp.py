"""runs/test.py --teacher hist --teacher-warp end to end on the device, in fresh child processes and without a data root: the synthetic
pair brings landmarks consistent with its label maps, the teacher image changes with the warp and only inside the face, and every row
the teacher run writes is still written."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run(tmp_path, name, *flags):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--res', '64', '--pairs', '1', '--batch-size', '1', '--ddim-steps', '5',
                        '--seed', '7', '--device-noise', '--out', str(out), '--teacher', 'hist', *flags],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out / 'makeupdiffuse_mi355x'


def test_runs_test_py_warps_the_teacher_image_of_a_synthetic_pair(tmp_path):
    from PIL import Image
    plain = run(tmp_path, 'plain')
    warped = run(tmp_path, 'warped', '--teacher-warp', '--teacher-warp-alphas', '1,1,1')
    names = sorted(os.listdir(warped))
    assert names == sorted(os.listdir(plain)) and 'ground_truth_0000.png' in names and 'sample_ddmp_0000.png' in names, names
    img = lambda root, n: np.asarray(Image.open(root / n)).astype(np.int32)
    assert np.array_equal(img(plain, 'control_src_0000.png'), img(warped, 'control_src_0000.png'))
    a, b = img(plain, 'ground_truth_0000.png'), img(warped, 'ground_truth_0000.png')
    changed = (a != b).any(-1)
    assert changed.mean() > 0.1                                            # the face is a third of the image
    # pixels whose 5 x 5 window (the default feather 2) holds no region of the SOURCE keep the alpha = 0 image
    import importlib.util
    import hist_match_ref as href
    import teacher_ref as tr
    spec = importlib.util.spec_from_file_location('mkd_runs_test', os.path.join(ROOT, 'runs', 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    regions = href.region_masks(cli.synthetic_seg(0, 64, True).numpy())
    masks = np.stack([regions[name] for name in tr.REGIONS])[:, None]
    outside = tr.window_counts(tr.region_ids(masks), 2).sum(0)[0] == 0
    assert outside.any() and not changed[outside].any() and changed[~outside].mean() > 0.3
