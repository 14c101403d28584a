"""fp32 torch restatement, on the CPU, of the face-parsing network (UPSTREAM zllrunning/face-parsing.PyTorch model.py / resnet.py:
BiSeNet with a ResNet-18 context path, inference path only) and a numpy restatement of the label head's arithmetic as include/mkd.h
states it.  Not the code under test: ``logits_bf16`` only EMULATES where the device rounds (folded convolution weights and every
stored activation to bf16), to size the error budget of the label tests."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F


@dataclass(frozen=True)
class Cfg:
    n_classes: int = 19
    widths: Tuple[int, int, int, int] = (64, 128, 256, 512)
    blocks: Tuple[int, int, int, int] = (2, 2, 2, 2)
    cp_channels: int = 128
    ffm_channels: int = 256
    bn_eps: float = 1e-5
    mean: Tuple[float, float, float] = (0.485, 0.456, 0.406)
    std: Tuple[float, float, float] = (0.229, 0.224, 0.225)


FULL = Cfg()
NARROW = Cfg(widths=(16, 32, 64, 128), blocks=(1, 1, 1, 1), cp_channels=32, ffm_channels=64)
# The committed fixture choice of the label tests: one seed per configuration, found by a search over seeds 0..399 (0..59 for the
# full configuration) for nets whose share of pixels with a top-two margin <= 4 E is below 0.4 % on the images the tests use
# (test_face_parser_host.py asserts <= 1 %).  E, the bf16 emulation's LARGEST error over all logits, is about 0.5 % of the standard
# deviation of all logits, but the margin between the two best classes of a pixel is itself a small part of that spread and passes
# through zero wherever two regions meet: over seeds 0..5, 9 - 46 % of the pixels lie within 4 E of a tie.  Scaling the classifier
# scales margins and E alike (LOGIT_SCALE therefore stays 1), and damping the residual branches (conv2 x 0.5: logits of spread 4 - 20
# instead of 50 - 500) does not change the picture: of 600 seeds per narrow configuration and 80 of the full one, none has a share
# <= 0.6 % together with a second region of >= 2 % of the map.  The condition therefore singles out nets in which ONE class wins
# nearly everywhere, and on these fixtures the margin-rule label comparison says little.  What tests the network is the logits
# comparison; what tests the labels pixel by pixel (the engine's logits layout, the parse size, the nearest resize) is
# test_parse_labels_equal_the_head_*, on generic seeds with several regions, against head_np on the logits the call itself returned.
SEEDS = {((1, 1, 1, 1), 19): 390, ((1, 1, 1, 1), 5): 42, ((2, 2, 2, 2), 19): 56, ((2, 2, 2, 2), 5): 102, 'full': 24}
LOGIT_SCALE = 1.0

LUT_PREPROCESS = [0, 1, 2, 3, 4, 5, 0, 11, 12, 0, 6, 8, 7, 9, 13, 0, 0, 10, 0]


def _bn(p, name, c):
    for f in ('weight', 'bias', 'running_mean', 'running_var'):
        p[f'{name}.{f}'] = (c,)


def param_spec(cfg: Cfg) -> Dict[str, Tuple[int, ...]]:
    """{upstream state-dict name: shape}, sorted by name"""
    w, cp, ff = cfg.widths, cfg.cp_channels, cfg.ffm_channels
    p: Dict[str, Tuple[int, ...]] = {'cp.resnet.conv1.weight': (w[0], 3, 7, 7)}
    _bn(p, 'cp.resnet.bn1', w[0])
    cin = w[0]
    for L in range(4):
        for i in range(cfg.blocks[L]):
            P = f'cp.resnet.layer{L + 1}.{i}'
            stride = 2 if (i == 0 and L > 0) else 1
            p[f'{P}.conv1.weight'] = (w[L], cin, 3, 3); _bn(p, f'{P}.bn1', w[L])
            p[f'{P}.conv2.weight'] = (w[L], w[L], 3, 3); _bn(p, f'{P}.bn2', w[L])
            if cin != w[L] or stride != 1:
                p[f'{P}.downsample.0.weight'] = (w[L], cin, 1, 1); _bn(p, f'{P}.downsample.1', w[L])
            cin = w[L]
    for arm, c in (('cp.arm16', w[2]), ('cp.arm32', w[3])):
        p[f'{arm}.conv.conv.weight'] = (cp, c, 3, 3); _bn(p, f'{arm}.conv.bn', cp)
        p[f'{arm}.conv_atten.weight'] = (cp, cp, 1, 1); _bn(p, f'{arm}.bn_atten', cp)
    for hd in ('cp.conv_head16', 'cp.conv_head32'):
        p[f'{hd}.conv.weight'] = (cp, cp, 3, 3); _bn(p, f'{hd}.bn', cp)
    p['cp.conv_avg.conv.weight'] = (cp, w[3], 1, 1); _bn(p, 'cp.conv_avg.bn', cp)
    p['ffm.convblk.conv.weight'] = (ff, w[1] + cp, 1, 1); _bn(p, 'ffm.convblk.bn', ff)
    p['ffm.conv1.weight'] = (ff // 4, ff, 1, 1)
    p['ffm.conv2.weight'] = (ff, ff // 4, 1, 1)
    p['conv_out.conv.conv.weight'] = (ff, ff, 3, 3); _bn(p, 'conv_out.conv.bn', ff)
    p['conv_out.conv_out.weight'] = (cfg.n_classes, ff, 1, 1)
    return dict(sorted(p.items()))


def param_count(cfg: Cfg) -> int:
    return sum(int(np.prod(s)) for s in param_spec(cfg).values())


GATE_CONVS = ('cp.arm16.conv_atten.weight', 'cp.arm32.conv_atten.weight', 'ffm.conv2.weight')


def init_state_dict(cfg: Cfg, seed: int, logit_scale: float = LOGIT_SCALE) -> Dict[str, torch.Tensor]:
    """He-normal convolutions N(0, 2 / fan_in): no layer dies, but every residual add about doubles the variance, so the logits
    have a spread of 50 - 500 (all finite, far inside bf16's range; the tests' bounds are relative); gamma in 1 +- 0.2, beta and
    running_mean in +- 0.2, running_var in [0.5, 1.5] (the fold is really exercised); the 1x1 convolutions in front of the sigmoids
    scaled by 4 so that the gates spread over about (0.1, 0.9); the classifier scaled by ``logit_scale`` (margins and the bf16
    error of a forward pass scale alike, so this only sets the logits' range)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape in param_spec(cfg).items():
        if name.endswith('running_var'):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith('running_mean') or name.endswith('.bias'):
            t = 0.4 * torch.rand(shape, generator=g) - 0.2
        elif len(shape) == 1:
            t = 0.8 + 0.4 * torch.rand(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
            if name in GATE_CONVS:
                t = t * 4.0
            if name == 'conv_out.conv_out.weight':
                t = t * float(logit_scale)
        sd[name] = t.float()
    return sd


def make_images(batch: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """smooth random RGB images in [0, 1] (low-resolution noise upsampled, plus a little pixel noise)"""
    g = torch.Generator().manual_seed(1000 + int(seed))
    low = torch.rand((batch, 3, H // 8, W // 8), generator=g)
    x = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False) + 0.1 * (torch.rand((batch, 3, H, W), generator=g) - 0.5)
    return x.clamp(0.0, 1.0).float().contiguous()


def _r(t: torch.Tensor, bf16: bool) -> torch.Tensor:
    return t.bfloat16().float() if bf16 else t


def fold(sd, conv: str, bn: str, eps: float):
    """W' = W g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps), fp32 (the library's order of operations)"""
    W = sd[conv + '.weight'].float()
    if not bn:
        return W, None
    s = sd[bn + '.weight'].float() / torch.sqrt(sd[bn + '.running_var'].float() + eps)
    return W * s[:, None, None, None], sd[bn + '.bias'].float() - sd[bn + '.running_mean'].float() * s


def _forward(sd, cfg: Cfg, x: torch.Tensor, bf16: bool) -> torch.Tensor:
    eps = cfg.bn_eps

    def cbr(t, conv, bn, stride=1, pad=1, relu=True, res=None, store=True):
        W, b = fold(sd, conv, bn, eps)
        if bf16:
            y = F.conv2d(t, _r(W, True), b, stride=stride, padding=pad)
        else:          # the unfolded form, as upstream computes it
            y = F.conv2d(t, sd[conv + '.weight'].float(), None, stride=stride, padding=pad)
            if bn:
                y = F.batch_norm(y, sd[bn + '.running_mean'].float(), sd[bn + '.running_var'].float(), sd[bn + '.weight'].float(),
                                 sd[bn + '.bias'].float(), False, 0.0, eps)
        if res is not None:
            y = y + res
        if relu:
            y = F.relu(y)
        return _r(y, bf16) if store else y

    def gate_vec(t, conv, bn, act):          # fp32 throughout on the device: folded weights are NOT rounded
        m = t.mean((2, 3), keepdim=True)
        W, b = fold(sd, conv, bn, eps)
        y = F.conv2d(m, W, b)
        return F.relu(y) if act == 'relu' else torch.sigmoid(y)

    mean = torch.tensor(cfg.mean).view(1, 3, 1, 1)
    std = torch.tensor(cfg.std).view(1, 3, 1, 1)
    t = (x.float() - mean) / std
    t = cbr(t, 'cp.resnet.conv1', 'cp.resnet.bn1', stride=2, pad=3)
    t = F.max_pool2d(t, 3, 2, 1)
    feats = []
    cin = cfg.widths[0]
    for L in range(4):
        for i in range(cfg.blocks[L]):
            P = f'cp.resnet.layer{L + 1}.{i}'
            stride = 2 if (i == 0 and L > 0) else 1
            h = cbr(t, P + '.conv1', P + '.bn1', stride=stride)
            sc = t
            if P + '.downsample.0.weight' in sd:
                sc = cbr(t, P + '.downsample.0', P + '.downsample.1', stride=stride, pad=0, relu=False)
            t = cbr(h, P + '.conv2', P + '.bn2', res=sc)
            cin = cfg.widths[L]
        feats.append(t)
    _, feat8, feat16, feat32 = feats
    avg = gate_vec(feat32, 'cp.conv_avg.conv', 'cp.conv_avg.bn', 'relu')
    f32_ = cbr(feat32, 'cp.arm32.conv.conv', 'cp.arm32.conv.bn')
    s32 = _r(f32_ * gate_vec(f32_, 'cp.arm32.conv_atten', 'cp.arm32.bn_atten', 'sigmoid') + avg, bf16)
    cp16 = cbr(F.interpolate(s32, scale_factor=2, mode='nearest'), 'cp.conv_head32.conv', 'cp.conv_head32.bn')
    f16_ = cbr(feat16, 'cp.arm16.conv.conv', 'cp.arm16.conv.bn')
    s16 = _r(f16_ * gate_vec(f16_, 'cp.arm16.conv_atten', 'cp.arm16.bn_atten', 'sigmoid') + cp16, bf16)
    cp8 = cbr(F.interpolate(s16, scale_factor=2, mode='nearest'), 'cp.conv_head16.conv', 'cp.conv_head16.bn')
    f = cbr(torch.cat((feat8, cp8), 1), 'ffm.convblk.conv', 'ffm.convblk.bn', pad=0)
    a = f.mean((2, 3), keepdim=True)
    a = torch.sigmoid(F.conv2d(F.relu(F.conv2d(a, sd['ffm.conv1.weight'].float())), sd['ffm.conv2.weight'].float()))
    fo = _r(f * a + f, bf16)
    o = cbr(fo, 'conv_out.conv.conv', 'conv_out.conv.bn')
    return cbr(o, 'conv_out.conv_out', '', pad=0, relu=False, store=False)


def logits(sd, cfg: Cfg, x: torch.Tensor) -> torch.Tensor:
    """[B,3,H,W] in [0,1] -> fp32 logits [B,n_classes,H/8,W/8]"""
    with torch.no_grad():
        return _forward(sd, cfg, x, False)


def logits_bf16(sd, cfg: Cfg, x: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        return _forward(sd, cfg, x, True)


def upsample(lg: torch.Tensor, P_h: int, P_w: int) -> torch.Tensor:
    """torch's bilinear align_corners=True upsample of the logits (the U of the label tests)"""
    return F.interpolate(lg.float(), size=(P_h, P_w), mode='bilinear', align_corners=True)


def head_np(lg: np.ndarray, P_h: int, P_w: int, out_h: int, out_w: int, lut=None, return_values: bool = False):
    """include/mkd.h mkd_parse_labels, operation by operation in np.float32: lg [B,C,h8,w8] -> labels uint8 [B,out_h,out_w]"""
    f32 = np.float32
    lg = np.asarray(lg, dtype=f32)
    B, C, h8, w8 = lg.shape
    oy, ox = np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64)
    py, px = (oy * P_h) // out_h, (ox * P_w) // out_w
    ry = f32(h8 - 1) / f32(P_h - 1) if (h8 > 1 and P_h > 1) else f32(0)
    rx = f32(w8 - 1) / f32(P_w - 1) if (w8 > 1 and P_w > 1) else f32(0)
    fy, fx = py.astype(f32) * ry, px.astype(f32) * rx
    y0 = np.minimum(fy.astype(np.int64), h8 - 1); y1 = np.minimum(y0 + 1, h8 - 1)
    x0 = np.minimum(fx.astype(np.int64), w8 - 1); x1 = np.minimum(x0 + 1, w8 - 1)
    wy = (fy - y0.astype(f32)).astype(f32)[None, None, :, None]
    wx = (fx - x0.astype(f32)).astype(f32)[None, None, None, :]
    v00 = lg[:, :, y0][:, :, :, x0]; v01 = lg[:, :, y0][:, :, :, x1]
    v10 = lg[:, :, y1][:, :, :, x0]; v11 = lg[:, :, y1][:, :, :, x1]
    top = (v00 + (wx * (v01 - v00)).astype(f32)).astype(f32)
    bot = (v10 + (wx * (v11 - v10)).astype(f32)).astype(f32)
    val = (top + (wy * (bot - top)).astype(f32)).astype(f32)
    lab = np.argmax(val, axis=1).astype(np.uint8)          # np.argmax returns the FIRST maximum
    if lut is not None:
        lab = np.asarray(lut, dtype=np.uint8)[lab]
    return (lab, val) if return_values else lab
