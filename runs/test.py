#!/usr/bin/env python
"""runs/test.py — inference entry point with the reference's shape (reference runs/test.py:27,59-64):
create_model(yaml) -> load_state_dict(ckpt) -> for batch in data: model.test_step(batch, i).

The reference hard-codes its constants in a "modify" block, needs the MT-Dataset, a trained checkpoint, CLIP and
PyTorch-Lightning; none exist offline, so every input is an argument here and the synthetic mode draws the batch
dict (src_img / ref_img / txt_emb) of SURVEY.md §8d.  One process per GPU; under torchrun the pair list is sharded.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from makeupdiffuse_amd import dist as mdist  # noqa: E402
from makeupdiffuse_amd.config import create_model, load_state_dict  # noqa: E402


def synthetic_seg(i, res, features=False):
    """a stand-in face-parsing map for pair i: background (0) outside an ellipse, hair (12) on its top, skin (1) inside;
    features: also eyes (4, 5) and lips (7, 9), the regions the makeup score reads"""
    g = torch.Generator().manual_seed(1213 + i)
    cy, cx = res * (0.5 + 0.1 * (torch.rand(2, generator=g) - 0.5))
    yy, xx = torch.meshgrid(torch.arange(res, dtype=torch.float32), torch.arange(res, dtype=torch.float32), indexing='ij')
    inside = ((yy - cy) / (0.4 * res)) ** 2 + ((xx - cx) / (0.3 * res)) ** 2 <= 1.0
    seg = torch.where(inside, torch.ones((), dtype=torch.uint8), torch.zeros((), dtype=torch.uint8))
    seg[inside & (yy < cy - 0.25 * res)] = 12
    if features:
        blob = lambda dy, dx, ry, rx: ((yy - cy - dy * res) / (ry * res)) ** 2 + ((xx - cx - dx * res) / (rx * res)) ** 2 <= 1.0
        seg[blob(-0.08, -0.11, 0.025, 0.05)] = 4
        seg[blob(-0.08, 0.11, 0.025, 0.05)] = 5
        seg[blob(0.18, 0.0, 0.035, 0.09) & (yy <= cy + 0.18 * res)] = 7
        seg[blob(0.18, 0.0, 0.035, 0.09) & (yy > cy + 0.18 * res)] = 9
    return seg


def synthetic_lms(i, res):
    """stand-in landmarks for pair i, consistent with synthetic_seg(i, res, features=True): the centre and the four extents of the face
    ellipse and of the eye and lip blobs, float32 [20, 2] in (y, x) pixels"""
    g = torch.Generator().manual_seed(1213 + i)
    cy, cx = (res * (0.5 + 0.1 * (torch.rand(2, generator=g) - 0.5))).tolist()
    pts = []
    for dy, dx, ry, rx in ((0.0, 0.0, 0.4, 0.3), (-0.08, -0.11, 0.025, 0.05), (-0.08, 0.11, 0.025, 0.05), (0.18, 0.0, 0.035, 0.09)):
        y, x = cy + dy * res, cx + dx * res
        pts += [(y, x), (y - ry * res, x), (y + ry * res, x), (y, x - rx * res), (y, x + rx * res)]
    return torch.tensor(pts, dtype=torch.float32)


def synthetic_batch(lo, hi, res, ctx_dim, with_seg=False, with_makeup_seg=False, with_lms=False):
    src, ref, txt = [], [], []
    for i in range(lo, hi):
        g = torch.Generator().manual_seed(5678 + i)
        src.append(torch.rand(1, 3, res, res, generator=g)); ref.append(torch.rand(1, 3, res, res, generator=g))
        g = torch.Generator().manual_seed(91011 + i)
        txt.append(torch.randn(1, 77, ctx_dim, generator=g))
    batch = {'src_img': torch.cat(src), 'ref_img': torch.cat(ref), 'txt_emb': torch.cat(txt),
             'txt': ['makeup transfer'] * (hi - lo), 'img_name': [f'{i:04d}&{i:04d}' for i in range(lo, hi)]}
    if with_seg:
        batch['nonmakeup_seg'] = torch.stack([synthetic_seg(i, res) for i in range(lo, hi)])
    if with_makeup_seg:
        batch['nonmakeup_seg'] = torch.stack([synthetic_seg(i, res, True) for i in range(lo, hi)])
        batch['makeup_seg'] = torch.stack([synthetic_seg(7000 + i, res, True) for i in range(lo, hi)])
    if with_lms:
        batch['nonmakeup_lms'] = torch.stack([synthetic_lms(i, res) for i in range(lo, hi)])
        batch['makeup_lms'] = torch.stack([synthetic_lms(7000 + i, res) for i in range(lo, hi)])
    return batch


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default=os.path.join(os.path.dirname(__file__), '..', 'diffmodels', 'test_diffusion_makeup.yaml'))
    ap.add_argument('--ckpt', default=None, help='upstream-named state_dict (.safetensors / tensor-only .ckpt); default: seeded random init')
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--batch-size', type=int, default=1)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--ddim-steps', type=int, default=None)
    ap.add_argument('--sampler', choices=('ddim', 'dpmpp', 'unipc'), default='ddim', help='dpmpp: DPM-Solver++ multistep on the DDIM step '
                    'grid (--ddim-steps is then its number of evaluations, typically 15-25); unipc: the UniPC predictor-corrector on '
                    'that grid, the solver for fewer evaluations still')
    ap.add_argument('--solver-order', type=int, choices=(1, 2, 3), default=2, help='order of --sampler dpmpp / unipc')
    ap.add_argument('--no-corrector', action='store_true', help='--sampler unipc: run the predictor alone')
    ap.add_argument('--only-mid-control', action='store_true')
    ap.add_argument('--out', default='./results')
    ap.add_argument('--data-root', default=None, help='folder with images/ and a pairs file (reference TestFixed_Dataset layout)')
    ap.add_argument('--pairs-file', default='test_0412.txt')
    ap.add_argument('--tokenizer', default=None, help='local CLIP tokenizer directory (vocab.json + merges.txt): prompts then go through the text encoder')
    ap.add_argument('--seed', type=int, default=None, help='start noise x_T drawn per PAIR from seed + pair index (results independent of '
                    'batch size / sharding); default: torch.randn like the reference')
    ap.add_argument('--device-noise', action='store_true', help='with --seed S: pair i draws EVERYTHING on the device from seed S + i (the '
                    'counter-based generator of makeupdiffuse_amd.noise: start latent, eta rows, the blend rows of --fix-background, the '
                    "encoder's posterior sample; with --photos the face's rank is the sub-stream), so a pair's result does not depend on the "
                    'batch, the sharding or what ran before; without this flag --seed keeps its host draw of the start latent')
    ap.add_argument('--txt-emb', default=None, help='.pt/.safetensors with a [1,77,768] tensor: the CLIP embedding of the prompt (offline stand-in)')
    ap.add_argument('--fix-background', action='store_true', help="keep the source's background, teeth and hair (label map "
                    "nonmakeup_seg from <data-root>/scgan_segs, a synthetic one otherwise; needs the first-stage encoder)")
    ap.add_argument('--makeup-score', action='store_true', help='score every decoded sample against its makeup reference: per region '
                    '(lip, skin, eye_left, eye_right) the L1 distance to its histogram match, one row per pair in <out>/makeup_score.csv '
                    '(label maps nonmakeup_seg / makeup_seg from <data-root>/scgan_segs, synthetic ones otherwise)')
    ap.add_argument('--region-refs', default=None, metavar='lip=NAME,eye=NAME,skin=NAME', help='region-wise transfer from several '
                    'references: after the usual passes every pair is also sampled with the named regions following these images '
                    '(names under <data-root>/images, the same for every pair; the rest of the face follows the pair\'s own reference) '
                    'and a samples_regions grid is written; needs <data-root>/scgan_segs')
    ap.add_argument('--region-strength', default=None, metavar='lip=0.7,...', help='strength per region of --region-refs (default 1)')
    ap.add_argument('--region-feather', type=int, default=1, help='box smoothing of the region weights, 0..4 latent pixels')
    ap.add_argument('--region-base', choices=('ref', 'source'), default='ref', help="what the rest of the face follows with --region-refs: "
                    "the pair's own reference, or the source itself (towards no makeup)")
    ap.add_argument('--region-paste-outside', action='store_true', help='with --region-refs and --region-base source: every pixel outside '
                    'the chosen regions keeps the source pixels (pasted after the decode, feathered by --paste-feather)')
    ap.add_argument('--paste-background', action='store_true', help="paste the source's pixels over background, teeth and hair into every "
                    'decoded sample (pixel space, after the decode; label map nonmakeup_seg from <data-root>/scgan_segs, a synthetic one '
                    'otherwise).  Independent of --fix-background; the two combine')
    ap.add_argument('--paste-feather', type=int, default=0, help='mix source and sample over this many image pixels on both sides of the '
                    'paste boundary, 0..16 (0: the hard mask of the reference)')
    ap.add_argument('--photos', action='store_true', help='after the usual passes, also transfer every pair at the photos\' NATIVE resolution: '
                    'the face box (<data-root>/boxes.txt, lines "name x0 y0 w h"; else the centred largest square) is crop-resized to --res on '
                    'the device, sampled once, and pasted back into the source photo with its fine detail kept; writes <out>/photos/<pair>.png')
    ap.add_argument('--max-faces', type=int, default=None, metavar='K', help='with --photos: group photos -- make up to K faces of every source '
                    'photo (largest first), each against the largest face of its reference; the faces come from --face-parser (connected '
                    'components of the parsed face classes) or from a boxes file that repeats an image name, one line per face')
    ap.add_argument('--own-pixels', action='store_true', help='with --photos --max-faces and faces from --face-parser: every face is pasted '
                    'onto its own pixels only (the pixels nearest to its component of the parsed map), so a crop that shows part of a '
                    'neighbouring face does not repaint it and a face beyond K keeps its bytes')
    ap.add_argument('--own-feather', type=int, default=2, metavar='N', help='with --own-pixels: blend neighbouring faces over N pixels of the '
                    'parsed map on both sides of their border, 0..16')
    ap.add_argument('--align-faces', action='store_true', help='with --photos --max-faces: tilted faces -- every face is cropped along a square '
                    'rotated by its roll (measured from the two eyes of the parsed map with --face-parser, or the sixth field of a boxes line, '
                    '"name x0 y0 w h angle" in degrees), so the model sees it upright, and pasted back along that square')
    ap.add_argument('--min-roll', type=float, default=5.0, metavar='DEG', help='with --align-faces: a face found by the parser whose measured '
                    'roll is below DEG degrees keeps its axis-aligned box')
    ap.add_argument('--photo-feather', type=int, default=8, help='fade the pasted face in over this many photo pixels at the box sides, 0..64')
    ap.add_argument('--guided-paste', action='store_true', help='with --photos: edge-aware paste -- the makeup difference is brought up to the '
                    'photo by joint bilateral upsampling under the photo\'s own luminance edges instead of bilinearly '
                    '(mkd_paste_photo_guided / mkd_paste_frame_guided), in every paste of the run')
    ap.add_argument('--guide-radius', type=int, default=1, metavar='R', help='with --guided-paste: the taps reach R + 1 model pixels per side, 0..2')
    ap.add_argument('--guide-sigma', type=float, default=8.0, metavar='S', help='with --guided-paste: the luminance distance, in 8-bit levels '
                    '(0.5 .. 1e6), at which a tap\'s weight has fallen to a half')
    ap.add_argument('--video', default=None, metavar='DIR', help='a clip INSTEAD of the pair passes: the image files of DIR, in sorted name '
                    'order, are the frames of one clip (no video container is read); every face keeps ONE noise sub-stream for the clip '
                    '(tracked identities, --seed is the clip\'s seed on the device), its crop is smoothed over time (--box-smooth) and the '
                    'makeup difference is filtered over time on the device (mkd_temporal_diff, --temporal-*).  The faces come from '
                    '--face-parser or from DIR/boxes.txt ("name x0 y0 w h" per face; the line of --video-ref\'s file name is the reference '
                    'face).  --max-faces (default 4), --align-faces, --guided-paste, --photo-feather and --res apply')
    ap.add_argument('--video-ref', default=None, metavar='IMAGE', help='with --video: the makeup reference, one photo for every face of the clip')
    ap.add_argument('--video-out', default=None, metavar='DIR', help='with --video: where the made-up frames go, under their own names '
                    '(default <out>/video)')
    ap.add_argument('--temporal-beta', type=float, default=0.8, metavar='B', help='with --video: the weight of the previous frame where '
                    'nothing moved, in (0, 0.95]; 0: no temporal filter')
    ap.add_argument('--temporal-tau', type=float, default=4.0, metavar='T', help='with --video: the mean luminance change, in 8-bit levels '
                    '(0.5 .. 1e6), at which that weight has fallen to a half')
    ap.add_argument('--temporal-radius', type=int, default=1, metavar='R', help='with --video: the luminance change is taken over a '
                    '(2 R + 1)^2 window of model pixels, 0..2')
    ap.add_argument('--video-motion', type=int, default=None, metavar='R', help='with --video and a temporal filter: block-matched motion in '
                    'front of the filter (mkd_motion_warp): the previous frame\'s state is fetched through one integer vector per block, '
                    'searched within +-R model pixels, 1..7 (default: off)')
    ap.add_argument('--video-motion-block', type=int, default=16, metavar='8|16', help='with --video-motion: the block side in model pixels')
    ap.add_argument('--video-motion-penalty', type=int, default=256, metavar='P', help='with --video-motion: what a vector must gain per pixel '
                    'of the block and pixel of displacement, in luminance units (256 = one grey level), 0..65280')
    ap.add_argument('--box-smooth', type=float, default=0.5, metavar='G', help='with --video: recursive smoothing of every track\'s crop, '
                    '0..0.95 (0: the crops as they were found)')
    ap.add_argument('--frame-batch', type=int, default=8, metavar='N', help='with --video: frames per push (all their faces are sampled together)')
    ap.add_argument('--face-parser', default=None, metavar='PATH|random', help='attach the face-parsing network (upstream face-parsing.PyTorch '
                    'state dict, e.g. 79999_iter.pth; "random": seeded random weights, for plumbing runs): label maps that --fix-background, '
                    '--paste-background, --makeup-score, --region-refs and --photos need and <data-root>/scgan_segs does not give are parsed '
                    'from the images, and --photos without a boxes file finds the face boxes itself')
    ap.add_argument('--teacher', choices=('hist',), default=None, help='the histogram-matching teacher (EleGANt pseudo ground truth at warp '
                    'weight 0, on the device): also write the reference\'s ground_truth / reconstruction / sample_ddmp rows, and with '
                    '--makeup-score the teacher image\'s score (label maps nonmakeup_seg / makeup_seg from <data-root>/scgan_segs, '
                    '--face-parser, or synthetic ones; needs the first-stage encoder)')
    ap.add_argument('--teacher-feather', type=int, default=2, metavar='F', help='with --teacher: box feather of the region weights, 0..8 image pixels')
    ap.add_argument('--teacher-start', type=float, default=None, metavar='TAU', help='with --teacher: start both passes from the diffused '
                    'teacher image and run only the last round(TAU * steps) steps, TAU in (0, 1] (the pair passes; not with --photos, --region-refs, --video)')
    ap.add_argument('--teacher-warp', action='store_true', help='with --teacher hist: add the landmark-warped term of the pseudo ground truth '
                    '(the reference warped onto the source by a thin-plate spline through the landmarks, blended in per region; landmarks from '
                    '<data-root>/lms/<name>.npy, synthetic ones without a data root; not with --photos, --region-refs, --video)')
    ap.add_argument('--teacher-warp-alphas', default=None, metavar='LIP,EYE,SKIN', help='with --teacher-warp: the blend weights in [0, 1] '
                    "(default: the reference's 0.1,0.8,0.3)")
    ap.add_argument('--teacher-points', choices=('masks',), default=None, help='with --teacher-warp: take the control points of the warped term '
                    'from the region masks instead of landmarks and solve the spline on the device: no <data-root>/lms is needed and '
                    '--photos is accepted (not with --region-refs, --video)')
    ap.add_argument('--teacher-point-dirs', type=int, choices=(8, 16), default=16, metavar='D', help='with --teacher-points masks: support '
                    'directions per region, 8 or 16 (4 (D + 1) control points per face)')
    ap.add_argument('--teacher-t-min', type=int, default=0, metavar='T', help='with --teacher: the sample_ddmp row diffuses to a timestep in [T, 1000)')
    ap.add_argument('--denoise-rows', action='store_true', help='also write the denoise rows of both passes (denoise_row*.png: the decoded '
                    'x0-predictions, samples as rows, x_T and the logged steps as columns), traced inside the sampling loop')
    ap.add_argument('--log-every-t', type=int, default=100, metavar='N', help='with --denoise-rows: log every table entry i with i %% N == 0 '
                    '(and the first executed step), the rule of the sampler\'s log_every_t')
    ap.add_argument('--guidance-rescale', type=float, default=0.0, metavar='PHI', help='guidance rescale of the guided pass, 0..1: per sample '
                    'and step the guided eps is scaled by PHI std(eps_cond) / std(eps_guided) + 1 - PHI (0: off)')
    ap.add_argument('--steps-list', default=None, metavar='20,50,...', help='per-sample requests in one batch: also sample every batch '
                    'with these step counts, cycled over its pairs, in ONE loop of the longest (samples_specs*.png)')
    ap.add_argument('--guidance-list', default=None, metavar='1.5,9,...', help='... and these guidance scales, cycled over the pairs '
                    '(alone: every pair at --ddim-steps)')
    return ap


def parse_number_list(text, cast, what):
    """'20,50' -> [20, 50]; SystemExit on anything else"""
    if text is None:
        return None
    try:
        vals = [cast(v) for v in text.split(',')]
    except ValueError:
        raise SystemExit(f'{what} takes comma-separated numbers, got {text!r}')
    if not vals:
        raise SystemExit(f'{what} is empty')
    return vals


def parse_region_map(text, cast=str):
    """'lip=a.png,eye=b.png' -> {'lip': 'a.png', 'eye': 'b.png'} (values through ``cast``)"""
    out = {}
    for part in (text or '').split(','):
        if not part.strip():
            continue
        if '=' not in part:
            raise ValueError(f"expected region=value, got '{part}'")
        k, v = part.split('=', 1)
        if k.strip() in out:
            raise ValueError(f"region '{k.strip()}' is given twice")
        out[k.strip()] = cast(v.strip())
    return out


def write_makeup_scores(path, names, out, first):
    """one makeup_score.csv row per pair and makeup_hist* entry of a test_step result; the first batch of a run rewrites the file"""
    from makeupdiffuse_amd.makeup_score import REGIONS
    with open(path, 'w' if first else 'a') as f:
        if first:
            f.write('pair,entry,' + ','.join(REGIONS) + '\n')
        for k in sorted(out):
            if k.startswith('makeup_hist'):
                for i, row in enumerate(out[k].tolist()):
                    f.write('%s,%s,%s\n' % (names[i], k, ','.join('%.6f' % v for v in row)))


IMAGE_EXTS = ('.png', '.jpg', '.jpeg', '.bmp', '.webp')


def check_video_args(args):
    """the --video flags -> None without --video, else dict(names, temporal, box_smooth, frame_batch, out); SystemExit on a bad one"""
    if not args.video:
        if (args.video_ref or args.video_out or args.temporal_beta != 0.8 or args.temporal_tau != 4.0 or args.temporal_radius != 1
                or args.box_smooth != 0.5 or args.frame_batch != 8 or args.video_motion is not None):
            raise SystemExit('--video-ref / --video-out / --temporal-* / --box-smooth / --frame-batch / --video-motion only apply with --video')
        return None
    from makeupdiffuse_amd import video
    if not args.video_ref:
        raise SystemExit('--video needs --video-ref IMAGE (the makeup reference of the clip)')
    if not os.path.isdir(args.video):
        raise SystemExit(f'--video: {args.video} is not a directory (the frames are its image files; no video container is read)')
    if not os.path.isfile(args.video_ref):
        raise SystemExit(f'--video-ref: {args.video_ref} is not a file')
    if args.photos or args.own_pixels:
        raise SystemExit('--video runs instead of the pair passes: --photos / --own-pixels do not combine with it')
    if args.seed is not None and not 0 <= args.seed < 2 ** 64:
        raise SystemExit('--video: --seed is the clip\'s 64-bit seed on the device, 0 .. 2^64 - 1')
    if not args.face_parser and not os.path.exists(os.path.join(args.video, 'boxes.txt')):
        raise SystemExit('--video needs --face-parser or <DIR>/boxes.txt (one line per face: name x0 y0 w h)')
    names = sorted(n for n in os.listdir(args.video) if n.lower().endswith(IMAGE_EXTS))
    if not names:
        raise SystemExit(f'--video: {args.video} holds no image file ({", ".join(IMAGE_EXTS)})')
    temporal = None
    try:
        if args.temporal_beta != 0.0:
            temporal = video.TemporalFilter(args.temporal_beta, args.temporal_tau, args.temporal_radius)
        gamma = video.check_box_smooth(args.box_smooth)
    except ValueError as e:
        raise SystemExit(f'--temporal-beta / --temporal-tau / --temporal-radius / --box-smooth: {e}')
    if args.frame_batch < 1:
        raise SystemExit('--frame-batch must be >= 1')
    motion = None
    if args.video_motion is None:
        if args.video_motion_block != 16 or args.video_motion_penalty != 256:
            raise SystemExit('--video-motion-block / --video-motion-penalty only apply with --video-motion R')
    else:
        if temporal is None:
            raise SystemExit('--video-motion compensates the temporal filter: it does not combine with --temporal-beta 0')
        try:
            motion = video.MotionSearch(args.video_motion, args.video_motion_block, args.video_motion_penalty)
        except ValueError as e:
            raise SystemExit(f'--video-motion / --video-motion-block / --video-motion-penalty: {e}')
    return dict(names=names, temporal=temporal, motion=motion, box_smooth=gamma, frame_batch=args.frame_batch,
                out=args.video_out or os.path.join(args.out, 'video'))


def clip_text(model, use_clip, txt_emb):
    """ONE row of text for a clip: the prompt through the text encoder, else --txt-emb, else the seeded stand-in of the pair passes"""
    if use_clip:
        return {'txt': ['makeup transfer']}
    g = torch.Generator().manual_seed(91011)
    return {'txt_emb': txt_emb if txt_emb is not None else torch.randn(1, 77, model.net_config.context_dim, generator=g)}


def run_video(model, args, opts, guided, text):
    """--video: the frames of opts['names'] through model.transfer_video -> the made-up frames under the same names in opts['out']"""
    import numpy as np
    from PIL import Image
    from makeupdiffuse_amd.photo import read_boxes_multi
    load = lambda path: torch.from_numpy(np.array(Image.open(path).convert('RGB'), dtype=np.uint8))
    frames = [load(os.path.join(args.video, n)) for n in opts['names']]
    ref = load(args.video_ref)
    src_boxes = ref_box = None
    bp = os.path.join(args.video, 'boxes.txt')
    K = 4 if args.max_faces is None else args.max_faces
    if os.path.exists(bp):          # a boxes file wins over the parser, as with --photos
        table = read_boxes_multi(bp)
        cut = (lambda b: b) if args.align_faces else (lambda b: b[:4])
        src_boxes = [[cut(b) for b in table.get(n, [])[:K]] for n in opts['names']]
        ref_lines = table.get(os.path.basename(args.video_ref))
        if ref_lines:
            ref_box = cut(ref_lines[0])
        elif not args.face_parser:
            raise SystemExit(f'--video: {bp} has no line for the reference {os.path.basename(args.video_ref)} and there is no --face-parser to find its face')
    out = model.transfer_video(frames, ref, frame_batch=opts['frame_batch'], src_boxes=src_boxes, ref_box=ref_box, seed=args.seed, size=args.res,
                               feather=args.photo_feather, max_faces=K, align=args.align_faces, min_roll=args.min_roll, guided_paste=guided,
                               temporal=opts['temporal'], box_smooth=opts['box_smooth'], batch=text, motion=opts['motion'])
    os.makedirs(opts['out'], exist_ok=True)
    for name, img in zip(opts['names'], out):
        Image.fromarray(img.cpu().numpy()).save(os.path.join(opts['out'], name))
    print(f'video: {len(out)} frames -> {opts["out"]}', flush=True)
    return out


def main():
    args = build_parser().parse_args()

    region_refs = parse_region_map(args.region_refs)
    region_strength = parse_region_map(args.region_strength, float) or None
    if region_refs:
        from makeupdiffuse_amd.regions import ordered
        ordered(region_refs)                              # unknown region names fail here, before the model is built
        if not args.data_root or not (args.face_parser or os.path.isdir(os.path.join(args.data_root, 'scgan_segs'))):
            raise SystemExit('--region-refs needs --data-root with images/ and scgan_segs/ or --face-parser (the label maps pick the regions)')
    elif region_strength or args.region_feather != 1 or args.region_base != 'ref' or args.region_paste_outside:
        raise SystemExit('--region-strength / --region-feather / --region-base / --region-paste-outside only apply with --region-refs')
    if args.region_paste_outside and args.region_base != 'source':
        raise SystemExit('--region-paste-outside needs --region-base source')
    if args.device_noise:
        if args.seed is None:
            build_parser().error('--device-noise needs --seed S (pair i draws from seed S + i)')
        if not 0 <= args.seed < 2 ** 64 - (1 << 40):
            build_parser().error('--device-noise: --seed must lie in 0 .. 2^64 - 2^40 (seed + pair index is a 64-bit seed)')
    if not 0 <= args.paste_feather <= 16:
        raise SystemExit('--paste-feather must be 0..16 image pixels')
    if args.paste_feather and not (args.paste_background or args.region_paste_outside):
        raise SystemExit('--paste-feather only applies with --paste-background or --region-paste-outside')
    if args.photos and not args.data_root:
        raise SystemExit('--photos needs --data-root with images/ and a pairs file (the photos are read at their own resolution)')
    if args.max_faces is not None:
        if not (args.photos or args.video):
            raise SystemExit('--max-faces only applies with --photos')
        if not 1 <= args.max_faces <= 64:
            raise SystemExit('--max-faces must be 1..64')
        if not args.video and not args.face_parser and not os.path.exists(os.path.join(args.data_root, 'boxes.txt')):
            raise SystemExit('--max-faces needs --face-parser or <data-root>/boxes.txt (one line per face)')
    if args.own_pixels:
        if not args.photos or args.max_faces is None:
            raise SystemExit('--own-pixels only applies with --photos --max-faces')
        if not args.face_parser or os.path.exists(os.path.join(args.data_root, 'boxes.txt')):
            raise SystemExit('--own-pixels needs the faces from --face-parser (no <data-root>/boxes.txt): a box has no component to own pixels')
        if not 0 <= args.own_feather <= 16:
            raise SystemExit('--own-feather must be 0..16 pixels of the parsed map')
    elif args.own_feather != 2:
        raise SystemExit('--own-feather only applies with --own-pixels')
    if args.align_faces:
        if not args.video and (not args.photos or args.max_faces is None):
            raise SystemExit('--align-faces only applies with --photos --max-faces')
        if not args.min_roll >= 0.0:
            raise SystemExit('--min-roll must be >= 0 degrees')
    elif args.min_roll != 5.0:
        raise SystemExit('--min-roll only applies with --align-faces (and --photos)')
    if not 0 <= args.photo_feather <= 64:
        raise SystemExit('--photo-feather must be 0..64 photo pixels')
    if args.photo_feather != 8 and not (args.photos or args.video):
        raise SystemExit('--photo-feather only applies with --photos')
    guided = None
    if args.guided_paste:
        if not (args.photos or args.video):
            raise SystemExit('--guided-paste only applies with --photos')
        from makeupdiffuse_amd.photo import GuidedPaste
        try:
            guided = GuidedPaste(args.guide_radius, args.guide_sigma)
        except ValueError as e:
            raise SystemExit(f'--guide-radius / --guide-sigma: {e}')
    elif args.guide_radius != 1 or args.guide_sigma != 8.0:
        raise SystemExit('--guide-radius / --guide-sigma only apply with --guided-paste')
    teacher_warp = None
    if args.teacher_warp_alphas is not None and not args.teacher_warp:
        raise SystemExit('--teacher-warp-alphas only applies with --teacher-warp')
    if args.teacher_points is None and args.teacher_point_dirs != 16:
        raise SystemExit('--teacher-point-dirs only applies with --teacher-points masks')
    if args.teacher_points is not None and not args.teacher_warp:
        raise SystemExit('--teacher-points only applies with --teacher-warp')
    if args.teacher_warp:
        if args.teacher is None:
            raise SystemExit('--teacher-warp / --teacher-warp-alphas only apply with --teacher hist')
        for on, flag in ((args.photos and args.teacher_points is None, '--photos'), (args.region_refs, '--region-refs'), (args.video, '--video')):
            if on:
                raise SystemExit(f'--teacher-warp is not combined with {flag} (those passes bring no landmarks)')
        teacher_warp = True
        if args.teacher_warp_alphas is not None:
            al = parse_number_list(args.teacher_warp_alphas, float, '--teacher-warp-alphas')
            if len(al) != 3 or not all(0.0 <= a <= 1.0 for a in al):
                raise SystemExit('--teacher-warp-alphas takes three numbers in [0, 1]: LIP,EYE,SKIN')
            teacher_warp = dict(lip=al[0], eye=al[1], skin=al[2])
    video_opts = check_video_args(args)
    if args.log_every_t < 1:
        raise SystemExit('--log-every-t must be >= 1')
    if args.log_every_t != 100 and not args.denoise_rows:
        raise SystemExit('--log-every-t only applies with --denoise-rows')
    if not 0.0 <= args.guidance_rescale <= 1.0:
        raise SystemExit('--guidance-rescale must lie in 0..1')
    if args.teacher is None:
        if args.teacher_feather != 2 or args.teacher_start is not None or args.teacher_t_min != 0:
            raise SystemExit('--teacher-feather / --teacher-start / --teacher-t-min only apply with --teacher hist')
    else:
        if not 0 <= args.teacher_feather <= 8:
            raise SystemExit('--teacher-feather must be 0..8 image pixels')
        if args.teacher_t_min < 0:
            raise SystemExit('--teacher-t-min must be >= 0')
        if args.teacher_start is not None:
            if not 0.0 < args.teacher_start <= 1.0:
                raise SystemExit('--teacher-start must lie in (0, 1]')
            for on, flag in ((args.fix_background, '--fix-background'), (args.denoise_rows, '--denoise-rows'),
                             (args.guidance_rescale != 0.0, '--guidance-rescale'), (args.steps_list or args.guidance_list, '--steps-list / --guidance-list'),
                             (args.video, '--video'), (args.photos, '--photos (transfer_photos takes teacher_start itself; the photo pass of this tool brings no reference label maps)'),
                             (args.region_refs, '--region-refs'), (args.seed is not None and not args.device_noise, '--seed without --device-noise (a given x_T)')):
                if on:
                    raise SystemExit(f'--teacher-start is not combined with {flag}')
    if args.no_corrector and args.sampler != 'unipc':
        raise SystemExit('--no-corrector only applies with --sampler unipc')
    if args.sampler == 'unipc' and args.fix_background:
        raise SystemExit('--sampler unipc has no masked form: --fix-background needs --sampler ddim or dpmpp')
    steps_list = parse_number_list(args.steps_list, int, '--steps-list')
    guidance_list = parse_number_list(args.guidance_list, float, '--guidance-list')
    if args.sampler == 'unipc' and (steps_list or guidance_list):
        raise SystemExit('--sampler unipc has no per-sample form: --steps-list / --guidance-list need --sampler ddim or dpmpp')
    if steps_list and not all(1 <= s <= 1024 for s in steps_list):
        raise SystemExit('--steps-list: every step count must lie in 1..1024')
    rank, world, local = mdist.init_from_env()
    model = create_model(args.config).cpu()
    if args.fix_background:
        if not getattr(model, 'first_stage_encoder', False):
            model.first_stage_encoder = True          # (configured on the device by .cuda() below)
        model.fix_background = True
    if args.makeup_score:
        model.makeup_score = True
    if args.teacher:
        model.first_stage_encoder = True          # (the reconstruction / sample_ddmp rows and the teacher start encode x_p)
        model.teacher, model.teacher_feather, model.teacher_t_min = args.teacher, args.teacher_feather, args.teacher_t_min
        model.teacher_start = args.teacher_start
        model.teacher_warp = teacher_warp
        model.teacher_points, model.teacher_point_dirs = args.teacher_points, args.teacher_point_dirs
    model.paste_background, model.paste_feather = args.paste_background, args.paste_feather
    if args.ddim_steps is not None:
        model.ddim_steps = args.ddim_steps
    model.sampler, model.solver_order = args.sampler, args.solver_order
    model.unipc_corrector = not args.no_corrector
    model.denoise_rows, model.log_every_t, model.guidance_rescale = args.denoise_rows, args.log_every_t, args.guidance_rescale
    if args.ckpt:
        model.load_state_dict(load_state_dict(args.ckpt, location='cpu'))
    torch.cuda.set_device(local)
    model.cuda(local)
    if not args.ckpt:
        model.engine.init_random(seed=0)
    model.only_mid_control = args.only_mid_control
    if args.face_parser:
        from makeupdiffuse_amd.face_parser import FaceParser
        parser = FaceParser(device=model.device)
        (parser.init_random(seed=0) if args.face_parser == 'random' else parser.load(args.face_parser)).finalize()
        model.face_parser = parser
    if args.tokenizer and model.cond_stage_model is not None:
        from makeupdiffuse_amd.clip import load_tokenizer
        model.cond_stage_model.tokenizer = load_tokenizer(args.tokenizer)
    use_clip = model.cond_stage_model is not None and model.cond_stage_model.tokenizer is not None
    if not use_clip:
        model.uncond_embedding = torch.zeros(1, 77, model.net_config.context_dim)   # stands for CLIP("") without a tokenizer
    model.eval()

    model.saved_dir = args.out
    model.test_pairs_file = os.path.join(args.out, f'test_pairs_rank{rank}.txt')
    dataset = None
    if args.data_root:
        from makeupdiffuse_amd.imageio import PairFolderDataset, collate
        dataset = PairFolderDataset(args.data_root, args.pairs_file, (args.res, args.res))
        args.pairs = len(dataset)
        if args.teacher_warp and args.teacher_points is None and not dataset.has_lms:
            raise SystemExit(f'--teacher-warp needs landmarks: {args.data_root}/lms/<name>.npy')
    photo_ds = None
    if args.photos:
        from makeupdiffuse_amd.photo import PhotoPairDataset, collate_photos
        photo_ds = PhotoPairDataset(args.data_root, args.pairs_file)
    txt_emb = None
    if args.txt_emb:
        t = load_state_dict(args.txt_emb)
        txt_emb = (next(iter(t.values())) if isinstance(t, dict) else t).float().reshape(1, 77, -1)
    if video_opts is not None:          # a clip instead of the pair passes; one process makes it up (a track's filter runs frame after frame)
        if rank == 0:
            run_video(model, args, video_opts, guided, clip_text(model, use_clip, txt_emb))
        mdist.barrier()
        return
    region_imgs = {r: dataset._load(name) for r, name in region_refs.items()}
    lo, hi = mdist.shard_range(args.pairs, rank, world)
    os.makedirs(args.out, exist_ok=True)
    model.on_test_epoch_start()
    for b0 in range(lo, hi, args.batch_size):
        b1 = min(hi, b0 + args.batch_size)
        if dataset is not None:
            batch = collate([dataset[i] for i in range(b0, b1)])
            if not use_clip:
                g = torch.Generator().manual_seed(91011)
                e = txt_emb if txt_emb is not None else torch.randn(1, 77, model.net_config.context_dim, generator=g)
                batch['txt_emb'] = e.expand(b1 - b0, -1, -1).contiguous()
        else:
            batch = synthetic_batch(b0, b1, args.res, model.net_config.context_dim, with_seg=(args.fix_background or args.paste_background) and not args.face_parser,
                                    with_makeup_seg=(args.makeup_score or bool(args.teacher)) and not args.face_parser, with_lms=args.teacher_warp and args.teacher_points is None)
            if use_clip:
                del batch['txt_emb']          # 'txt' -> tokenizer -> mkd_clip_encode
        x_T = None
        # --device-noise: pair i's seed is --seed + i wherever the pair is drawn for; the model then draws everything on the device
        seeded = {'seeds': [args.seed + i for i in range(b0, b1)]} if args.device_noise else {}
        if args.seed is not None and not args.device_noise:
            h8 = args.res // 8
            x_T = torch.cat([torch.randn(1, model.channels, h8, h8, generator=torch.Generator().manual_seed(args.seed + i))
                             for i in range(b0, b1)]).cuda(local)
        out = model.test_step(batch, b0, x_T=x_T, **seeded)
        model.on_test_batch_end(out, batch, b0)
        if region_refs:
            for r, img in region_imgs.items():
                batch['region_ref_' + r] = img.unsqueeze(0).expand(b1 - b0, -1, -1, -1).contiguous()
            reg = model.transfer_regions(batch, {r: 'region_ref_' + r for r in region_refs}, strengths=region_strength,
                                         feather=args.region_feather, x_T=x_T, base=args.region_base,
                                         paste_outside=args.region_paste_outside, **seeded)
            out['samples_regions_latent'] = reg['samples_latent'].detach().cpu()
            if 'samples' in reg:
                out['samples_regions'] = torch.clamp(reg['samples'].detach().cpu(), -1.0, 1.0)
                model.save_local({'samples_regions': out['samples_regions']}, b0)
        if steps_list or guidance_list:
            from makeupdiffuse_amd.batching import SampleSpec
            n = b1 - b0
            specs = [SampleSpec(steps=(steps_list[i % len(steps_list)] if steps_list else model.ddim_steps),
                                guidance=(guidance_list[i % len(guidance_list)] if guidance_list else 1.0), order=model.solver_order)
                     for i in range(n)]
            sp = model.transfer_specs(batch, specs, x_T=x_T, **seeded)
            out['samples_specs_latent'] = sp['samples_latent'].detach().cpu()
            if 'samples' in sp:
                out['samples_specs'] = torch.clamp(sp['samples'].detach().cpu(), -1.0, 1.0)
                model.save_local({'samples_specs': out['samples_specs']}, b0)
        if photo_ds is not None:
            from PIL import Image
            items = collate_photos([photo_ds[i] for i in range(b0, b1)])
            text = {k: batch[k] for k in ('txt_emb', 'txt') if k in batch}
            find = bool(args.face_parser) and not photo_ds.boxes          # no boxes file: the parser finds the faces
            if args.max_faces is None:
                photos = model.transfer_photos(items['src_photo'], items['ref_photo'], None if find else items['src_box'], None if find else items['ref_box'],
                                               src_segs=items.get('src_seg'), feather=args.photo_feather, x_T=x_T, size=args.res, batch=text,
                                               guided_paste=guided, **seeded)
            else:
                K = args.max_faces
                ref_boxes = items['ref_box']
                tilt = dict(oriented=True, min_roll=args.min_roll) if args.align_faces else {}          # (then the faces are photo.Frame's)
                if find:          # (a reference in which the parser finds no face keeps its centred largest square)
                    look = lambda ps, k: model.face_parser.find_faces([p.cuda(local) for p in ps], max_faces=k, parse_size=model.parse_size,
                                                                      lut=model.parser_lut, **tilt)
                    faces = look(items['src_photo'], K)
                    ref_boxes = [f[0] if f else b for f, b in zip(look(items['ref_photo'], 1), ref_boxes)]
                else:          # the lines of the source's name, else the one box the single-face run uses; a line's angle counts with --align-faces
                    cut = (lambda b: b) if args.align_faces else (lambda b: b[:4])
                    faces = [[cut(b) for b in photo_ds.faces.get(photo_ds.pairs[i][0], [items['src_box'][i - b0]])[:K]] for i in range(b0, b1)]
                    ref_boxes = [cut(photo_ds.faces.get(photo_ds.pairs[i][1], [ref_boxes[i - b0]])[0]) for i in range(b0, b1)]
                x_F = None
                if args.seed is not None and not args.device_noise:          # one start latent per face: seed + pair index, then the face's rank
                    h8 = args.res // 8
                    x_F = [torch.randn(1, model.channels, h8, h8, generator=torch.Generator().manual_seed((args.seed + i) * 64 + k))
                           for i in range(b0, b1) for k in range(len(faces[i - b0]))]
                    x_F = torch.cat(x_F).cuda(local) if x_F else None
                own = dict(own_pixels=True, own_feather=args.own_feather) if args.own_pixels else {}
                if args.align_faces:
                    own.update(align=True, min_roll=args.min_roll)
                # (--own-pixels: the model finds the same faces again, with their owner map; the count above sizes the start latents)
                photos, faces = model.transfer_photos(items['src_photo'], items['ref_photo'], None if args.own_pixels else faces, ref_boxes,
                                                      src_segs=items.get('src_seg'), feather=args.photo_feather, x_T=x_F, size=args.res, batch=text,
                                                      max_faces=K, return_faces=True, guided_paste=guided, **own, **seeded)
                print(f'[rank {rank}] faces per photo: {[len(f) for f in faces]}', flush=True)
            if guided is not None:
                print(f'[rank {rank}] guided paste: radius {guided.radius}, sigma {guided.sigma:g}', flush=True)
            os.makedirs(os.path.join(args.out, 'photos'), exist_ok=True)
            for name, img in zip(items['img_name'], photos):
                Image.fromarray(img.cpu().numpy()).save(os.path.join(args.out, 'photos', name + '.png'))
        if args.makeup_score:
            write_makeup_scores(os.path.join(args.out, f'makeup_score_rank{rank}.csv' if world > 1 else 'makeup_score.csv'),
                                batch.get('img_name') or [str(i) for i in range(b0, b1)], out, first=b0 == lo)
        torch.save({k: v for k, v in out.items() if isinstance(v, torch.Tensor)},
                   os.path.join(args.out, f'latents_{b0:04d}.pt'))
        print(f'[rank {rank}] pairs {b0}..{min(hi, b0 + args.batch_size) - 1}: ' +
              ', '.join(f'{k} {tuple(v.shape)}' for k, v in out.items() if isinstance(v, torch.Tensor)), flush=True)
    mdist.barrier()


if __name__ == '__main__':
    main()
