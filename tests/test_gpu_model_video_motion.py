"""-m gpu: block-matched motion in TestDiffuseModel.video_session / transfer_video, on the small model and the stub parser of
tests/test_gpu_model_video.py: on a still clip motion changes no byte (every vector is zero), the made-up frames do not depend on how
the clip is split into pushes, and runs/test.py --video-motion writes the frames."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from makeupdiffuse_amd import video
from test_gpu_model_photo import S, model  # noqa: F401  (the module-scoped small model; this module gets an instance of its own)
from test_gpu_model_video import CROSS, REF_MAP, SEED, StubParser, data, m  # noqa: F401  (the fixtures of the video tests)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_on_a_still_clip_motion_changes_no_byte(m, data):  # noqa: F811
    out = {}
    for name, ms in (('off', None), ('on', video.MotionSearch())):
        m.reset_conditioning_cache()
        m.face_parser = StubParser(REF_MAP, CROSS[:1].expand(4, -1, -1))
        sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=4, face_batch=8, batch=data['text'], motion=ms)
        out[name] = (sess, sess.push([data['frames'][0]] * 4))
    off, on = out['off'][0].state, out['on'][0].state
    assert off.launches == 4 and off.motion_launches == 0 and off.last_vectors is None
    assert on.launches == 4 and on.motion_launches == on.launches
    assert tuple(on.last_vectors.shape) == (2, S // 16, S // 16, 2) and not on.last_vectors.any()
    assert not torch.equal(out['on'][1][0].cpu(), data['frames'][0])
    for f, (a, b) in enumerate(zip(out['on'][1], out['off'][1])):
        assert torch.equal(a, b), f'frame {f}: {int((a != b).sum())} bytes differ from the session without motion'
    assert [r._fields for r in out['on'][0].last] == [r._fields for r in out['off'][0].last]          # FrameRecord keeps its fields


def test_the_frames_do_not_depend_on_the_split_into_pushes(m, data):  # noqa: F811
    ms = video.MotionSearch(3, 8, 64)

    def run(split):
        m.reset_conditioning_cache()
        parts, f0 = [], 0
        for n in split:
            parts.append(CROSS[f0:f0 + n])
            f0 += n
        m.face_parser = StubParser(REF_MAP, *parts)
        sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=4, face_batch=8, batch=data['text'], motion=ms)
        got, vecs, f0 = [], [], 0
        for n in split:
            got += sess.push(data['frames'][f0:f0 + n])
            f0 += n
        assert sess.state.motion_launches == sess.state.launches == 4
        return got, sess.state.last_vectors.cpu()

    whole, vec = run((4,))
    assert vec.any()                                          # (the frames are unrelated noise: the search does pick vectors)
    parts, vec1 = run((1, 1, 1, 1))
    assert torch.equal(vec1, vec)
    for f, (a, b) in enumerate(zip(parts, whole)):
        assert torch.equal(a, b), f'frame {f}: {int((a != b).sum())} bytes differ from the clip pushed at once'


def test_runs_test_py_video_motion_writes_the_frames(tmp_path):
    """runs/test.py --video ... --video-motion 3 in a fresh child process on a 3-frame directory with a boxes file"""
    from PIL import Image
    rng = np.random.default_rng(32)
    clip = tmp_path / 'clip'
    os.makedirs(clip)
    names = ['f000.png', 'f001.png', 'f002.png']
    frames = {n: rng.integers(0, 256, (80, 112, 3), dtype=np.uint8) for n in names}
    for n, arr in frames.items():
        Image.fromarray(arr).save(clip / n)
    Image.fromarray(rng.integers(0, 256, (70, 60, 3), dtype=np.uint8)).save(tmp_path / 'ref.png')
    (clip / 'boxes.txt').write_text(''.join(f'{n} {8 + i} 10 48 48\n' for i, n in enumerate(names)) + 'ref.png 4 6 50 50\n')
    out = tmp_path / 'out'
    argv = ['--video', str(clip), '--video-ref', str(tmp_path / 'ref.png'), '--video-out', str(out), '--res', '64', '--ddim-steps', '2', '--seed', '9',
            '--photo-feather', '3', '--frame-batch', '2', '--video-motion', '3', '--video-motion-block', '8', '--video-motion-penalty', '128',
            '--out', str(tmp_path / 'results')]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py')] + argv, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == names and 'video: 3 frames' in r.stdout
    for n in names:
        g = np.asarray(Image.open(out / n))
        assert g.shape == frames[n].shape and (g != frames[n]).any()
    # the flags are checked before a model is built
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py')] + argv + ['--temporal-beta', '0'], capture_output=True, text=True,
                         timeout=900, cwd=str(tmp_path))
    assert bad.returncode != 0 and '--video-motion' in bad.stderr
