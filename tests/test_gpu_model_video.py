"""-m gpu: TestDiffuseModel.video_session / transfer_video on the small model of tests/test_gpu_model_photo.py at S = 64, frames of
96 x 128 and a stub parser with drawn label maps (the set-up of tests/test_gpu_model_faces.py).  With the switches off a push is the
photo path byte for byte; a track keeps its noise when the detector swaps the faces; a still clip stays still; the temporal filter
is in the path; and the pasted bytes are the numpy chain tests/video_ref.py -> tests/photo_ref.py / tests/photo_guided_ref.py on
the decoded images the session reports."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import photo_guided_ref as pgr
import photo_ref as pr
import video_ref as vr
from gpu_util import DEV
from makeupdiffuse_amd import noise, photo, video
from test_gpu_model_photo import S, model  # noqa: F401  (the module-scoped small model; this module gets an instance of its own)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = 64                                    # parse size of the stub's label maps
HW, REF_HW = (96, 128), (80, 100)
SEED = 4242


class StubParser:
    """duck-typed face parser: parse() hands out the label maps of ``seq`` in turn"""

    def __init__(self, *seq):
        self.seq, self.n = [s.to(DEV) for s in seq], 0

    def parse(self, img01, out_size=None, lut=None, return_logits=False):
        maps = self.seq[self.n % len(self.seq)]
        self.n += 1
        assert out_size is None and tuple(img01.shape) == (maps.shape[0], 3, PS, PS)
        return maps


def face_map(*faces):
    """a label map with one square blob (centre row, centre col, side) per face"""
    m = torch.zeros(PS, PS, dtype=torch.uint8)
    for cr, cc, side in faces:
        r0, c0 = cr - side // 2, cc - side // 2
        m[r0:r0 + side, c0:c0 + side] = 1
    return m


A = lambda side: (30, 16, side)
B = lambda side: (32, 46, side)
# two faces whose areas cross over between frames 1 and 2: find_faces (largest first) swaps their order
CROSS = torch.stack([face_map(A(14), B(11)), face_map(A(13), B(12)), face_map(A(12), B(13)), face_map(A(11), B(14))])
ONE = torch.stack([face_map(A(14)), face_map(A(13)), face_map(A(12)), face_map(A(13))])
REF_MAP = face_map((35, 35, 30))[None]


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(191)
    rand = lambda hw: torch.randint(0, 256, (hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    return dict(frames=[rand(HW) for _ in range(4)], ref=rand(REF_HW), text={'txt_emb': torch.randn(1, 77, 64, generator=g)})


@pytest.fixture()
def m(model):  # noqa: F811
    model.parse_size = PS
    model.reset_conditioning_cache()
    yield model
    model.face_parser, model.parse_size = None, 512


def spy_on_start_latents(monkeypatch):
    """every start latent a sampling pass draws: (the Seeds, the tensor) per noise.normal call on STREAM_START"""
    calls, real = [], noise.normal

    def normal(seeds, shape, *, stream, **kw):
        out = real(seeds, shape, stream=stream, **kw)
        if stream == noise.STREAM_START:
            calls.append((seeds, out))
        return out

    monkeypatch.setattr(noise, 'normal', normal)
    return calls


def box_mask(box):
    x0, y0, bw, bh = box
    inside = np.zeros(HW, bool)
    inside[y0:y0 + bh, x0:x0 + bw] = True
    return inside


def test_with_the_switches_off_a_push_is_the_photo_path(m, data):
    m.face_parser = StubParser(REF_MAP, ONE)
    sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=1, face_batch=4, temporal=None, box_smooth=0, batch=data['text'])
    got = sess.push(data['frames'])
    assert sess.state is None and [r.tracks for r in sess.last] == [[0]] * 4
    m.reset_conditioning_cache()
    m.face_parser = StubParser(ONE, REF_MAP.expand(4, -1, -1))
    want, faces = m.transfer_photos(data['frames'], [data['ref']] * 4, feather=3, size=S, batch={'txt_emb': data['text']['txt_emb'].expand(4, -1, -1)},
                                    max_faces=1, face_batch=4, seeds=[SEED] * 4, return_faces=True)
    assert [r.regions for r in sess.last] == faces                                     # the regions as they were found: integer boxes
    for g, w, p in zip(got, want, data['frames']):
        assert g.dtype == torch.uint8 and g.device.type == 'cuda' and torch.equal(g, w) and not torch.equal(g.cpu(), p)


def test_identity_follows_the_face_not_the_rank(m, data, monkeypatch):
    calls = spy_on_start_latents(monkeypatch)
    shape = (4, S // 8, S // 8)

    def run(split):
        m.reset_conditioning_cache()
        parts, f0 = [], 0
        for n in split:
            parts.append(CROSS[f0:f0 + n])
            f0 += n
        m.face_parser = StubParser(REF_MAP, *parts)
        sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=4, face_batch=8, batch=data['text'])
        del calls[:]
        records, out, f0, drawn, subs = [], [], 0, [], []
        for n in split:
            c0 = len(calls)
            out += sess.push(data['frames'][f0:f0 + n])
            records += sess.last
            f0 += n
            assert len(calls) - c0 == len(sess.chunks) and all(batch == 8 for _, batch in sess.chunks)          # every chunk at face_batch
            for (sd, x), (real, _) in zip(calls[c0:], sess.chunks):          # a ragged chunk is filled up with repeats of its last item
                assert sd.subs[real:] == sd.subs[real - 1:real] * (8 - real)
                drawn.append(x[:real])                                                  # frame-major, in the detector's order
                subs += sd.subs[:real]
        assert all(sd.seeds == (SEED,) * len(sd) for sd, _ in calls)
        return records, torch.cat(drawn), subs, out

    records, drawn, subs, whole = run((4,))
    assert [r.tracks for r in records] == [[0, 1], [0, 1], [1, 0], [1, 0]]               # the detector swapped them, the tracks did not
    assert subs == [t for r in records for t in r.tracks] and tuple(drawn.shape) == (8, *shape)
    want = {k: noise.normal([SEED], shape, stream=noise.STREAM_START, subs=[k], device=DEV)[0] for k in (0, 1)}
    assert not torch.equal(want[0], want[1])
    for j, k in enumerate(subs):
        assert torch.equal(drawn[j].view(torch.int32), want[k].view(torch.int32)), f'item {j} (track {k})'
    assert all(isinstance(reg, photo.Frame) for r in records[1:] for reg in r.regions)   # smoothed crops
    assert records[0].regions == records[0].raw and [r.restarted for r in records] == [[True, True]] + [[False, False]] * 3
    # the host decisions and the noise do not depend on how the clip is split into pushes; nor do the made-up frames, because with a
    # seed every chunk is sampled at face_batch
    for split in ((1, 3), (2, 2)):
        rec2, drawn2, subs2, parts = run(split)
        assert [(r.tracks, r.restarted, r.raw, r.regions) for r in rec2] == [(r.tracks, r.restarted, r.raw, r.regions) for r in records]
        assert subs2 == subs and torch.equal(drawn2.view(torch.int32), drawn.view(torch.int32))
        for f, (a, b) in enumerate(zip(parts, whole)):
            assert torch.equal(a, b), f'split {split}, frame {f}: {int((a != b).sum())} bytes differ from the clip pushed at once'


def still_clip(m, data, n_frames, face_batch):
    """n identical frames with two faces, default temporal and box_smooth -> (the session, the made-up frames)"""
    m.reset_conditioning_cache()
    m.face_parser = StubParser(REF_MAP, CROSS[:1].expand(n_frames, -1, -1))
    sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=4, face_batch=face_batch, batch=data['text'])
    return sess, sess.push([data['frames'][0]] * n_frames)


def test_a_still_clip_stays_still(m, data):
    """4 identical frames in ONE chunk (face_batch = 2 faces x 4): all four frames come out with equal bytes, the first (which has
    no previous frame) included, and they equal frame 0 of a one-frame push: its two faces are sampled at face_batch too (the chunk
    filled up with repeats), so the GEMM planner picks the tiles it picked for the clip.  Sampled at ANOTHER batch (2) the same noise
    gave decoded images up to 1.5e-01 away (max |value| 3.3; bf16 network, random weights, guidance 9) and 5932 other bytes."""
    s4, got = still_clip(m, data, 4, 8)
    assert s4.state.launches == 4 and [r.tracks for r in s4.last] == [[0, 1]] * 4 and s4.chunks == [(8, 8)]
    assert not torch.equal(got[0].cpu(), data['frames'][0])
    assert all(torch.equal(g, got[0]) for g in got)
    s1, one = still_clip(m, data, 1, 8)
    assert s1.chunks == [(2, 8)]
    dec4, dec1 = s4.last[0].decoded, s1.last[0].decoded
    print(f'clip against its one-frame push: crops equal {torch.equal(s4.last[0].src01, s1.last[0].src01)}, decoded max |difference| '
          f'{float((dec4 - dec1).abs().max()):.3e} (max |value| {float(dec1.abs().max()):.3f}), {int((got[0] != one[0]).sum())} pasted bytes differ')
    assert torch.equal(got[0], one[0])


def test_the_filter_is_in_the_path(m, data):
    rng = np.random.default_rng(77)
    f0 = data['frames'][0]
    f1 = torch.from_numpy(np.clip(f0.numpy().astype(np.int64) + rng.integers(0, 4, f0.shape), 0, 255).astype(np.uint8))          # + 0..3 grey levels
    change = {}
    for name, temporal in (('on', video.TemporalFilter(beta=0.8)), ('off', None)):
        m.reset_conditioning_cache()
        m.face_parser = StubParser(REF_MAP, ONE[:1].expand(2, -1, -1))
        sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=1, face_batch=2, temporal=temporal, box_smooth=0, batch=data['text'])
        a, b = sess.push([f0, f1])
        inside = box_mask(sess.last[0].regions[0])
        assert sess.last[1].regions == sess.last[0].regions
        change[name] = float(np.abs(a.cpu().numpy().astype(np.int64) - b.cpu().numpy().astype(np.int64))[inside].mean())
    print(f'mean |byte change| of the made-up face between the two frames: filter on {change["on"]:.4f}, off {change["off"]:.4f}')
    assert change['on'] < change['off']


@pytest.mark.parametrize('guided', [None, photo.GuidedPaste(1, 8.0)], ids=['bilinear', 'guided'])
def test_pasted_bytes_are_the_numpy_chain(m, data, guided):
    filt = video.TemporalFilter(0.8, 4.0, 1)
    m.face_parser = StubParser(REF_MAP, CROSS)
    sess = m.video_session(data['ref'], seed=SEED, size=S, feather=3, max_faces=4, face_batch=8, guided_paste=guided, temporal=filt, box_smooth=0,
                           batch=data['text'])
    got = sess.push(data['frames'])
    state = {}
    for f, (rec, g) in enumerate(zip(sess.last, got)):
        dec, s01, flt = rec.decoded.cpu().numpy(), rec.src01.cpu().numpy(), rec.filtered.cpu().numpy()
        out = data['frames'][f].numpy().copy()
        new_state = {}
        for k, (tid, box) in enumerate(zip(rec.tracks, rec.regions)):                     # rank by rank, largest first
            assert len(box) == 4
            prev = state.get(tid, (None, None))
            t_out, D, Y = vr.step(dec[k], s01[k], prev[0], prev[1], filt.beta, filt.tau, filt.radius)
            new_state[tid] = (D, Y)
            assert np.array_equal(flt[k].view(np.uint32), t_out.view(np.uint32)), f'frame {f}, track {tid}: the filtered sample'
            out = pr.paste(out, box, t_out, s01[k], 3) if guided is None else pgr.paste(out, box, t_out, s01[k], 3, guided.radius, guided.sigma)
        state = new_state
        assert f == 0 or not np.array_equal(flt, dec)
        assert np.array_equal(g.cpu().numpy(), out), f'frame {f}: {int((g.cpu().numpy() != out).sum())} bytes differ from the numpy chain'


def test_refusals_need_no_sampling(m, data):
    m.face_parser = StubParser(REF_MAP)
    with pytest.raises(ValueError, match='own_pixels'):
        m.video_session(data['ref'], own_pixels=True)
    with pytest.raises(ValueError, match='per-track references'):
        m.video_session([data['ref'], data['ref']])
    for kw, word in ((dict(temporal=(0.8, 4.0, 1)), 'TemporalFilter'), (dict(box_smooth=0.99), 'box_smooth'), (dict(max_faces=0), 'max_faces'),
                     (dict(face_batch=0), 'face_batch'), (dict(tracker=object()), 'FaceTracker')):
        with pytest.raises(ValueError, match=word):
            m.video_session(data['ref'], **kw)
    assert m.face_parser.n == 0


def test_runs_test_py_video_writes_the_frames_of_the_api(tmp_path):
    """runs/test.py --video in a fresh child process on a 3-frame directory with a boxes file: 3 files under the frames' names, equal to
    transfer_video on the model the script builds (the default yaml, seeded random weights)"""
    from PIL import Image
    rng = np.random.default_rng(31)
    clip = tmp_path / 'clip'
    os.makedirs(clip)
    names = ['f002.png', 'f000.png', 'f001.png']                                       # written out of order: sorted names are the clip's order
    frames = {n: rng.integers(0, 256, (80, 112, 3), dtype=np.uint8) for n in names}
    for n, arr in frames.items():
        Image.fromarray(arr).save(clip / n)
    ref = rng.integers(0, 256, (70, 60, 3), dtype=np.uint8)
    Image.fromarray(ref).save(tmp_path / 'ref.png')
    boxes = {'f000.png': [(8, 10, 48, 48), (62, 20, 40, 40)], 'f001.png': [(64, 21, 40, 40), (9, 10, 48, 48)], 'f002.png': [(10, 11, 48, 48)]}
    (clip / 'boxes.txt').write_text(''.join(f'{n} %d %d %d %d\n' % b for n in sorted(boxes) for b in boxes[n]) + 'ref.png 4 6 50 50\n')
    out = tmp_path / 'out'
    argv = ['--video', str(clip), '--video-ref', str(tmp_path / 'ref.png'), '--video-out', str(out), '--res', '64', '--ddim-steps', '2', '--seed', '9',
            '--photo-feather', '3', '--frame-batch', '2', '--temporal-tau', '6', '--out', str(tmp_path / 'results')]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py')] + argv, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(out)) == sorted(names) and 'video: 3 frames' in r.stdout
    wrote = [np.asarray(Image.open(out / n)) for n in sorted(names)]
    # the API on the model the script builds
    spec = importlib.util.spec_from_file_location('runs_test_cli_video', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args(argv)
    mdl = mod.create_model(args.config).cpu()
    mdl.paste_background, mdl.paste_feather, mdl.ddim_steps, mdl.sampler, mdl.solver_order, mdl.unipc_corrector = False, 0, 2, 'ddim', 2, True
    mdl.denoise_rows, mdl.log_every_t, mdl.guidance_rescale = False, 100, 0.0
    mdl.cuda(0)
    mdl.engine.init_random(seed=0)
    mdl.only_mid_control = False
    mdl.uncond_embedding = torch.zeros(1, 77, mdl.net_config.context_dim)
    mdl.eval()
    want = mdl.transfer_video([torch.from_numpy(frames[n]) for n in sorted(names)], torch.from_numpy(ref), frame_batch=2,
                                src_boxes=[boxes[n] for n in sorted(names)], ref_box=(4, 6, 50, 50), seed=9, size=64, feather=3, max_faces=4,
                                temporal=video.TemporalFilter(0.8, 6.0, 1), box_smooth=0.5, batch=mod.clip_text(mdl, False, None))
    for n, w, g in zip(sorted(names), want, wrote):
        assert g.shape == frames[n].shape and np.array_equal(g, w.cpu().numpy()), n
        assert (g != frames[n]).any()
