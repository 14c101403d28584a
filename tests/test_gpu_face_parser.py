"""-m gpu: the face-parsing network on the device (include/mkd.h mkd_parser_*): the ReLU epilogue code, the stem, the channel gate,
the gate apply and the label head one by one, the whole network against the fp32 restatement of tests/face_parser_ref.py, the
handle's state rules.  Shapes are the smallest at which each kernel can still go wrong (more than one workgroup, odd tile
remainders, every path of the code)."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import face_parser_ref as R
from gpu_util import DEV, L, P, assert_close_bf16, bf, rel_l2, sync
from makeupdiffuse_amd import face_parser as fp

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_MISSING = -1, -3, -5


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype).cpu()


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = bits(a) != bits(b)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ'


# ---- ReLU in the shared GEMM epilogue (act = 4) ------------------------------------------------------------------------------------

def _gemm(A, W, bias, R_, act, splitk, conv=None):
    lib = L()
    N, K = W.shape
    if conv is None:
        M, cv = A.shape[0], (0, 0, 0, 0, 0, 0, 0, 1, 0)
        lda = K
    else:
        B, Hin, Win, Cin, stride = conv
        Ho, Wo = Hin // stride, Win // stride
        M, cv, lda = B * Ho * Wo, (1, B, Hin, Win, Cin, Ho, Wo, stride, 0), Cin
    out = torch.full((M, N), float('nan'), device=DEV, dtype=torch.bfloat16)
    rc = lib.mkd_gemm_bf16(P(A), lda, P(W), K, P(bias), None, 0, 1, P(R_), 0 if R_ is None else N, 1.0, act, P(out), N, 0, M, N, K, *cv, splitk, None)
    assert rc == 0, lib.mkd_last_error()
    sync()
    return out


def _relu_case(kind, with_res):
    g = torch.Generator().manual_seed(17)
    if kind == 'linear':
        M, N, K, conv = 96, 64, 64, None
        A = bf(torch.randn(M, K, generator=g))
        W = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
        ref = A.float() @ W.float().t()
    else:
        _, Cin, stride, H, Wd, Cout = kind
        B = 2
        x = bf(torch.randn(B, H, Wd, Cin, generator=g))
        w4 = bf(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
        A, W = x, w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
        ref = F.conv2d(x.float().permute(0, 3, 1, 2), w4.float(), None, stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
        M, N, K, conv = ref.shape[0], Cout, 9 * Cin, (B, H, Wd, Cin, stride)
    bias = torch.randn(N, generator=g).to(DEV)
    R_ = bf(torch.randn(M, N, generator=g)) if with_res else None
    ref = ref + bias + (R_.float() if with_res else 0.0)
    geom = (M, N, K, 1, conv[1], conv[2], conv[3], conv[1] // conv[4], conv[2] // conv[4], conv[4], 0) if conv else (M, N, K, 0, 0, 0, 0, 0, 0, 1, 0)
    return A, W, bias, R_, conv, ref, geom


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('kind', ['linear', ('conv', 16, 1, 8, 12, 32), ('conv', 16, 2, 8, 12, 32), ('conv', 128, 1, 16, 16, 64)],
                         ids=['linear', 'conv_s1', 'conv_s2', 'conv_s1_lds_staged'])
def test_relu_epilogue(kind, with_res):
    """act = 4 equals max(act = 0, 0) BIT FOR BIT (rounding is monotone) on every tile configuration that takes the shape, with and
    without split-K, and meets the per-kernel bound against torch.  The 8 x 12 maps fit no LDS-staged conv tile (their spatial tiles
    are 16 or W columns wide and must hold 64 / 128 / 256 pixels); the 16 x 16 map with Cin = 128 (two channel chunks, so split-K 2
    splits) fits them, and the test asserts that LDS-staged configurations really ran."""
    lib = L()
    A, W, bias, R_, conv, ref, geom = _relu_case(kind, with_res)
    ran = staged_ran = 0
    staged = C.c_int(0)
    for cfg in range(lib.mkd_gemm_tile_info(-1, None, None, None, None)):
        if not lib.mkd_gemm_cfg_supported(cfg, *geom):
            continue
        lib.mkd_gemm_tile_info(cfg, None, None, C.byref(staged), None)
        staged_ran += staged.value
        for splitk in (1, 2):
            lib.mkd_gemm_force_tile(cfg)
            try:
                plain = _gemm(A, W, bias, R_, 0, splitk, conv)
                relu = _gemm(A, W, bias, R_, 4, splitk, conv)
            finally:
                lib.mkd_gemm_force_tile(-1)
            same_bits(relu, torch.clamp_min(plain.float(), 0.0).bfloat16(), f'cfg {cfg} splitk {splitk}')
            assert_close_bf16(relu, torch.relu(ref), what=f'relu cfg {cfg} splitk {splitk}')
            ran += 1
    assert ran >= 2
    if kind != 'linear' and kind[3:5] == (16, 16):
        assert staged_ran >= 3, f'only {staged_ran} LDS-staged conv tile configurations accepted the shape'
    for splitk in (1, 2):          # and on the plan the library picks itself
        same_bits(_gemm(A, W, bias, R_, 4, splitk, conv), torch.clamp_min(_gemm(A, W, bias, R_, 0, splitk, conv).float(), 0.0).bfloat16(), 'auto plan')


# ---- stem -----------------------------------------------------------------------------------------------------------------------------

def _stem(x, w, bn, C0, cfg=R.FULL):
    """device stem on images x [B,3,H,W] with conv weight w [C0,3,7,7] and BatchNorm tensors bn -> bf16 NHWC [B,H/4,W/4,C0]"""
    sd = {'c.weight': w, 'b.weight': bn[0], 'b.bias': bn[1], 'b.running_mean': bn[2], 'b.running_var': bn[3]}
    Wf, b = R.fold(sd, 'c', 'b', cfg.bn_eps)
    wp = Wf.permute(2, 3, 1, 0).reshape(147, C0).bfloat16().contiguous().to(DEV)          # [(ky*7+kx)*3+c][C0]
    B, _, H, Wd = x.shape
    half = torch.empty((B, H // 2, Wd // 2, C0), device=DEV, dtype=torch.bfloat16)
    y = torch.full((B, H // 4, Wd // 4, C0), float('nan'), device=DEV, dtype=torch.bfloat16)
    mean, std = (C.c_float * 3)(*cfg.mean), (C.c_float * 3)(*cfg.std)
    xd, bd = x.to(DEV).contiguous(), b.to(DEV).contiguous()
    rc = L().mkd_parser_stem(P(xd), P(wp), P(bd), mean, std, P(half), P(y), B, H, Wd, C0, None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return y, wp.float().cpu().reshape(7, 7, 3, C0).permute(3, 2, 0, 1).contiguous(), b


def _stem_ref(x, w_rounded, b, cfg=R.FULL):
    t = (x - torch.tensor(cfg.mean).view(1, 3, 1, 1)) / torch.tensor(cfg.std).view(1, 3, 1, 1)
    return F.max_pool2d(F.relu(F.conv2d(t, w_rounded, b, stride=2, padding=3)), 3, 2, 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize('C0', [16, 64])
@pytest.mark.parametrize('H,W', [(64, 64), (64, 96)])
def test_stem(H, W, C0):
    g = torch.Generator().manual_seed(H + W + C0)
    x = torch.rand(2, 3, H, W, generator=g)
    x[1] = 0.5          # constant: border pixels differ from the interior only through the zero padding of the NORMALISED image
    w = torch.randn(C0, 3, 7, 7, generator=g) * math.sqrt(2.0 / 147)
    bn = (0.8 + 0.4 * torch.rand(C0, generator=g), 0.4 * torch.rand(C0, generator=g) - 0.2, 0.4 * torch.rand(C0, generator=g) - 0.2,
          0.5 + torch.rand(C0, generator=g))
    y, w_rounded, b = _stem(x, w, bn, C0)
    ref = _stem_ref(x, w_rounded, b)
    assert_close_bf16(y, ref, what=f'stem {H}x{W} C0={C0}')
    # the constant image: a mean folded into the bias would make every pixel equal; the padded border must differ, and match
    const = y[1].float().cpu()
    assert (const[0, 0] - const[H // 8, W // 8]).abs().max() > 1e-3
    assert_close_bf16(y[1], ref[1], what='stem, constant image')


# ---- channel gate ---------------------------------------------------------------------------------------------------------------------

def _gate(x, w1, b1, act1, w2=None, b2=None, act2=0):
    B, Pn, Cn = x.shape
    n_out = (w2 if w2 is not None else w1).shape[0]
    out = torch.full((B, n_out), float('nan'), device=DEV)
    rc = L().mkd_channel_gate(P(x), Cn, B, Pn, Cn, P(w1), P(b1), w1.shape[0], act1, P(w2), P(b2), 0 if w2 is None else w2.shape[0], act2, P(out), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return out


def _gate_ref(x, w1, b1, act1, w2=None, b2=None, act2=0):
    """fp64 restatement -> (value, magnitude): the magnitude of an output is the sum of the ABSOLUTE terms of the sums it comes from
    (|x| averaged, |mean| . |W|, |b|), carried through the second mat-vec; the activations do not stretch an error (slope <= 1).
    fp32 rounding of a sum is relative to that magnitude, not to a result that cancellation made small."""
    f = {0: lambda v: v, 1: lambda v: v.clamp_min(0), 2: torch.sigmoid}
    xd, w1d = x.double().cpu(), w1.double().cpu()
    m, ma = xd.mean(1), xd.abs().mean(1)
    b1d = torch.zeros(w1d.shape[0], dtype=torch.float64) if b1 is None else b1.double().cpu()
    h, ha = f[act1](m @ w1d.t() + b1d), ma @ w1d.abs().t() + b1d.abs()
    if w2 is None:
        return h, ha
    w2d = w2.double().cpu()
    b2d = torch.zeros(w2d.shape[0], dtype=torch.float64) if b2 is None else b2.double().cpu()
    return f[act2](h @ w2d.t() + b2d), ha @ w2d.abs().t() + b2d.abs()


@pytest.mark.parametrize('Cn', [32, 128, 512])
@pytest.mark.parametrize('pixels', [1, 4, 4096])
def test_channel_gate(Cn, pixels):
    g = torch.Generator().manual_seed(Cn + pixels)
    x3 = bf(torch.randn(3, pixels, Cn, generator=g) + 0.5)
    n1 = 24
    w1 = (torch.randn(n1, Cn, generator=g) / math.sqrt(Cn)).to(DEV); b1 = (0.3 * torch.randn(n1, generator=g)).to(DEV)
    w2 = (torch.randn(Cn, n1, generator=g) / math.sqrt(n1)).to(DEV)
    for args in ((w1, b1, 2), (w1, b1, 1), (w1, None, 1, w2, None, 2)):
        got3 = _gate(x3, *args)
        want, mag = _gate_ref(x3, *args)
        err = (got3.double().cpu() - want).abs()
        assert (err <= 1e-5 * torch.maximum(mag, want.abs())).all(), (err / torch.maximum(mag, want.abs())).max()          # rtol 1e-5 of the sums, no atol
        same_bits(_gate(x3, *args), got3, 'two runs')
        for b in range(3):
            same_bits(_gate(x3[b:b + 1].contiguous(), *args)[0], got3[b], f'batch-1 call on sample {b}')


# ---- gate apply -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('Cn', [32, 128])
@pytest.mark.parametrize('u', [0, 1])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_gate_apply(mode, u, Cn):
    g = torch.Generator().manual_seed(mode * 7 + u * 3 + Cn)
    B, h, w = 2, 4, 6
    x = bf(torch.randn(B, h, w, Cn, generator=g))
    a = torch.rand(B, Cn, generator=g).to(DEV)
    up = lambda t: t.repeat_interleave(1 << u, 1).repeat_interleave(1 << u, 2)
    if mode == 0:
        add_t = torch.randn(B, Cn, generator=g).to(DEV); add = add_t[:, None, None, :]
    elif mode == 1:
        add_t = bf(torch.randn(B, h, w, Cn, generator=g)); add = up(add_t.float())
    else:
        add_t, add = None, up(x.float())
    y = torch.full((B, h << u, w << u, Cn), float('nan'), device=DEV, dtype=torch.bfloat16)
    rc = L().mkd_gate_apply_bf16(P(x), Cn, P(a), mode, P(add_t), Cn, P(y), Cn, B, h, w, Cn, u, None)
    assert rc == 0, L().mkd_last_error()
    sync()
    same_bits(y, (up(x.float()) * a[:, None, None, :] + add).bfloat16(), f'gate apply mode {mode} u {u}')


# ---- head -----------------------------------------------------------------------------------------------------------------------------

def _head(lg_nchw, layout, P_hw, out_hw, lut):
    """mkd_parse_labels on NCHW strides or on an NHWC copy with 20 columns; the labels buffer is pre-filled with 255 and has a guard tail"""
    B, nc, h8, w8 = lg_nchw.shape
    if layout == 'nchw':
        t = lg_nchw.to(DEV).contiguous()
        s = (h8 * w8, w8, 1, nc * h8 * w8)
    else:
        t = torch.full((B, h8, w8, 20), float('nan'), device=DEV)
        t[..., :nc] = lg_nchw.permute(0, 2, 3, 1).to(DEV)
        s = (1, w8 * 20, 20, h8 * w8 * 20)
    n = B * out_hw[0] * out_hw[1]
    buf = torch.full((n + 64,), 255, device=DEV, dtype=torch.uint8)
    lut_c = None if lut is None else (C.c_uint8 * nc)(*lut)
    rc = L().mkd_parse_labels(P(t), *s, B, nc, h8, w8, P_hw[0], P_hw[1], out_hw[0], out_hw[1], lut_c, P(buf), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    buf = buf.cpu().numpy()
    assert (buf[n:] == 255).all(), 'bytes beyond batch * out_h * out_w were written'
    return buf[:n].reshape(B, *out_hw)


HEAD_GEOM = [((1, 1), (8, 8)), ((8, 8), (64, 64)), ((8, 12), (64, 96))]


@pytest.mark.parametrize('nc', [5, 19])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc20'])
@pytest.mark.parametrize('hw8,P_hw', HEAD_GEOM)
def test_head(hw8, P_hw, layout, nc):
    rng = np.random.default_rng(hw8[1] * 31 + nc)
    lg = rng.standard_normal((2, nc, *hw8)).astype(np.float32) * 3.0
    lut_all = [(7 * i + 3) % 200 + 50 for i in range(nc)]          # values 50..249: an unwritten byte (255) or an unmapped class (< 50) shows
    for out_hw in (P_hw, (40, 56), (128, 192)):
        for lut in (None, lut_all):
            got = _head(torch.from_numpy(lg), layout, P_hw, out_hw, lut)
            want = R.head_np(lg, *P_hw, *out_hw, lut=lut)
            assert (got == want).all(), f'{int((got != want).sum())} labels differ, out {out_hw}, lut {lut is not None}'
            assert (got != 255).all()


@pytest.mark.parametrize('layout', ['nchw', 'nhwc20'])
def test_head_ties(layout):
    """all classes equal: class 0 / lut[0]; two equal maxima: the lower index wins"""
    nc = 19
    flat = np.full((1, nc, 8, 12), 0.25, dtype=np.float32)
    assert (_head(torch.from_numpy(flat), layout, (64, 96), (64, 96), None) == 0).all()
    assert (_head(torch.from_numpy(flat), layout, (64, 96), (40, 56), list(range(9, 9 + nc))) == 9).all()
    two = np.random.default_rng(5).standard_normal((1, nc, 8, 12)).astype(np.float32)
    two[:, 4] = 9.0; two[:, 11] = 9.0          # exactly representable, equal after every interpolation step
    assert (_head(torch.from_numpy(two), layout, (64, 96), (128, 192), None) == 4).all()


# ---- the whole network ----------------------------------------------------------------------------------------------------------------

_parsers = {}


def _parser(cfg, seed):
    """one finalized device parser per (config, seed), with its state dict"""
    key = (cfg, seed)
    if key not in _parsers:
        sd = R.init_state_dict(cfg, seed)
        p = fp.FaceParser(fp.FaceParserConfig(**dataclasses.asdict(cfg)), device=DEV)
        p.load_state_dict(sd).finalize()
        _parsers[key] = (p, sd)
    return _parsers[key]


def _check_whole(cfg, seed, B, H, W):
    p, sd = _parser(cfg, seed)
    x = R.make_images(B, H, W, seed=B)
    Lr = R.logits(sd, cfg, x)
    E = (R.logits_bf16(sd, cfg, x) - Lr).abs().max().item()
    labels, lg = p.parse(x.to(DEV), lut=None, return_logits=True)
    sync()
    Ld = lg.cpu()
    assert torch.isfinite(Ld).all()
    rel = rel_l2(Ld, Lr)
    cos = F.cosine_similarity(Ld.flatten().double(), Lr.flatten().double(), dim=0).item()
    D = (Ld - Lr).abs().max().item()
    print(f'whole net {cfg.blocks} nc={cfg.n_classes} B={B} {H}x{W}: rel-L2 {rel:.3e} cos {cos:.6f} D {D:.4g} E {E:.4g}')
    assert rel <= 2e-2 and cos >= 0.9995, (rel, cos)
    assert D <= 2 * E, f'device error {D:.4g} exceeds twice the bf16 emulation error {E:.4g}'
    U = R.upsample(Lr, H, W)
    ref_lab = U.argmax(1)
    dev_lab = labels.cpu().long()
    diff = dev_lab != ref_lab
    share = diff.float().mean().item()
    print(f'    labels: {int(diff.sum())} of {diff.numel()} differ ({share:.4%})')
    if diff.any():
        gap = U.gather(1, ref_lab[:, None])[:, 0] - U.gather(1, dev_lab[:, None])[:, 0]
        lim = 2 * D + 4 * np.spacing(np.float32(U.abs().max().item()))
        assert (gap[diff] <= lim).all(), f'a differing label is {gap[diff].max().item():.4g} below the winner, more than 2 D = {2 * D:.4g} allows'
    assert share <= 0.01, share
    return p, x, labels, lg


@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (3, 64, 96)])
@pytest.mark.parametrize('nc', [19, 5])
@pytest.mark.parametrize('blocks', [(1, 1, 1, 1), (2, 2, 2, 2)])
def test_whole_net_narrow(blocks, nc, B, H, W):
    """logits within the project's whole-evaluation bounds of the fp32 restatement (rel-L2 <= 2e-2, cosine >= 0.9995);
    D = max |device - restatement| <= 2 E, E the error of the restatement's own bf16 emulation; labels differ from the restatement's
    only where its upsampled logits are within 2 D (+ 4 ulp) of the winner, on at most 1 % of the map."""
    cfg = dataclasses.replace(R.NARROW, blocks=blocks, n_classes=nc)
    p, x, labels, lg = _check_whole(cfg, R.SEEDS[(blocks, nc)], B, H, W)
    same_bits(p.logits(x.to(DEV)), lg, 'mkd_parser_parse logits vs mkd_parser_logits')


def _check_labels_exact(cfg, seed, B, H, W, outs):
    """labels of mkd_parser_parse == the numpy head on the logits the SAME call returned, bit for bit: checks, pixel by pixel on maps
    with several regions, the strides the engine hands its head (fp32 NHWC with padded columns), the parse size and the nearest
    resize -- with no margin condition, because both sides read the same logits"""
    p, _ = _parser(cfg, seed)
    x = R.make_images(B, H, W, seed=B).to(DEV)
    for out in outs:
        for lut in (None, list(fp.LUT_SEG) if cfg.n_classes == 19 else list(range(40, 40 + cfg.n_classes))):
            labels, lg = p.parse(x, out_size=out, lut=lut, return_logits=True)
            sync()
            want = R.head_np(lg.cpu().numpy(), H, W, *out, lut=lut)
            got = labels.cpu().numpy()
            assert got.shape == want.shape and (got == want).all(), f'{int((got != want).sum())} of {want.size} labels differ, out {out}, lut {lut is not None}'
            if lut is None:
                count = np.sort(np.bincount(got.reshape(-1), minlength=cfg.n_classes))[::-1]
                assert count[1] >= 0.02 * got.size, f'the fixture has one region only: {count[:4]}'          # a head that ignores position would pass otherwise


@pytest.mark.parametrize('blocks,nc,seed,B,H,W', [((1, 1, 1, 1), 19, 0, 2, 64, 64), ((2, 2, 2, 2), 19, 0, 3, 64, 96), ((1, 1, 1, 1), 5, 2, 3, 64, 96)])
def test_parse_labels_equal_the_head_on_the_returned_logits(blocks, nc, seed, B, H, W):
    """generic seeds whose label maps have several regions; square and non-square, at the image size, smaller and larger"""
    _check_labels_exact(dataclasses.replace(R.NARROW, blocks=blocks, n_classes=nc), seed, B, H, W, [(H, W), (40, 56), (2 * H, 2 * W)])


def test_parse_labels_equal_the_head_full_size():
    """the real configuration at 512 x 512 on a seed whose map has a dozen classes (14)"""
    _check_labels_exact(R.FULL, 14, 1, 512, 512, [(512, 512), (200, 312)])


def test_whole_net_batch_rows_and_reallocation():
    """row b of a batch-3 call = a batch-1 call on sample b, bit for bit; calls with alternating (batch, H, W) reallocate correctly"""
    cfg = dataclasses.replace(R.NARROW, blocks=(2, 2, 2, 2), n_classes=19)
    p, _ = _parser(cfg, R.SEEDS[((2, 2, 2, 2), 19)])
    x3 = R.make_images(3, 64, 96, seed=3).to(DEV)
    x2 = R.make_images(2, 64, 64, seed=2).to(DEV)
    l3, g3 = p.parse(x3, return_logits=True)
    l2, g2 = p.parse(x2, return_logits=True)
    for b in range(3):
        lb, gb = p.parse(x3[b:b + 1], return_logits=True)
        same_bits(gb[0], g3[b], f'logits of sample {b}')
        same_bits(lb[0], l3[b], f'labels of sample {b}')
    l3b, g3b = p.parse(x3, return_logits=True)          # grow again after the smaller calls
    same_bits(g3b, g3, 'batch 3 again')
    same_bits(l3b, l3, 'batch 3 labels again')
    same_bits(p.parse(x2, return_logits=True)[1], g2, 'batch 2 again')
    assert p.launches() > 0 and p.flops(64, 64) > 0


def test_whole_net_full_size():
    """the real configuration at 512 x 512, batch 1: the same two assertions"""
    _check_whole(R.FULL, R.SEEDS['full'], 1, 512, 512)


# ---- state handling -------------------------------------------------------------------------------------------------------------------

def test_state_handling():
    cfg = dataclasses.replace(R.NARROW, n_classes=5)
    sd = R.init_state_dict(cfg, 1)
    p = fp.FaceParser(fp.FaceParserConfig(**dataclasses.asdict(cfg)), device=DEV)
    x = R.make_images(1, 64, 64, seed=9).to(DEV)
    lab = torch.empty((1, 64, 64), device=DEV, dtype=torch.uint8)
    assert p.lib.mkd_parser_parse(p._h, P(x), 1, 64, 64, 64, 64, None, P(lab), None, None) == ERR_STATE          # before finalize
    missing = 'cp.arm16.bn_atten.running_var'
    for k, v in sd.items():
        if k != missing:
            p.load_weight(k, v)
    assert p.lib.mkd_parser_finalize(p._h) == ERR_MISSING and missing in p.lib.mkd_last_error().decode()
    p.load_weight(missing, sd[missing])
    p.load_weight('conv_out16.conv.conv.weight', torch.zeros(4, 4, 3, 3))          # training-only heads: accepted and ignored
    p.load_weight('cp.resnet.bn1.num_batches_tracked', torch.zeros(()))
    with pytest.raises(Exception):
        p.load_weight('cp.resnet.conv1.weight', torch.zeros(3, 3, 7, 7))              # wrong shape
    with pytest.raises(Exception):
        p.load_weight('cp.nothing.weight', torch.zeros(3))                            # unknown
    p.finalize()
    g1 = p.logits(x)
    assert rel_l2(g1, R.logits(sd, cfg, x.cpu())) <= 2e-2
    # a weight loaded after finalize: another finalize is needed, and gives the new net's output
    sd2 = dict(sd); sd2['conv_out.conv_out.weight'] = -sd['conv_out.conv_out.weight']
    p.load_weight('conv_out.conv_out.weight', sd2['conv_out.conv_out.weight'])
    assert p.lib.mkd_parser_parse(p._h, P(x), 1, 64, 64, 64, 64, None, P(lab), None, None) == ERR_STATE
    p.finalize()
    same_bits(p.logits(x), -g1, 'negated classifier')
    p.close()


# ---- model and harness ----------------------------------------------------------------------------------------------------------------

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8: 8 x 8 latent -> 64 x 64
S = 64


@pytest.fixture(scope='module')
def model():
    """the SMALL model of the model tests with a random narrow parser attached (19 classes, parse size 64)"""
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    from oracle import nets, vae
    ocfg = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64, hint_widths=tuple(HINT_WIDTHS))
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    parser, _ = _parser(dataclasses.replace(R.NARROW, blocks=(1, 1, 1, 1), n_classes=19), 7)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, ddim_steps=2,
                         unconditional_guidance_scale=9, paste_background=True, face_parser=parser, parse_size=S)
    m.load_state_dict({**nets.init_state_dict(ocfg, seed=31), **vae.init_state_dict(vcfg, seed=32)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


def test_model_transfer_photos_parses_the_crop(model):
    """transfer_photos(src_segs=None) = the same call given parse(crop) as label maps through the existing path, bit for bit"""
    from makeupdiffuse_amd import photo
    g = torch.Generator().manual_seed(78)
    rand = lambda h, w: torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV)
    src, ref = [rand(150, 203), rand(97, 130)], [rand(120, 90), rand(70, 64)]
    src_boxes, ref_boxes = [(30, 10, 130, 130), (0, 5, 90, 88)], [(5, 20, 80, 80), (0, 0, 64, 64)]
    kw = dict(feather=0, x_T=torch.randn(2, 4, 8, 8, generator=g), size=S, batch={'txt_emb': torch.randn(2, 77, 64, generator=g)})
    crops = list(photo.crop_resize(src, src_boxes, S, want_u8=True).u8)          # crop first ...
    ident = [(0, 0, S, S)] * 2
    labels = model.parse_images(photo.crop_resize(crops, ident, S).img01)         # ... parse ...
    assert labels.shape == (2, S, S) and labels.dtype == torch.uint8 and int(labels.max()) <= 13
    want = model.transfer_photos(crops, ref, ident, ref_boxes, src_segs=list(labels), **kw)          # ... and feed the label maps
    got = model.transfer_photos(crops, ref, ident, ref_boxes, src_segs=None, **kw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    full = model.transfer_photos(src, ref, src_boxes, ref_boxes, src_segs=None, **kw)          # photos of their own size run too
    assert [tuple(p.shape) for p in full] == [(150, 203, 3), (97, 130, 3)]


def test_model_log_results_parses_missing_label_maps(model):
    g = torch.Generator().manual_seed(96)
    batch = {'src_img': torch.rand(2, 3, S, S, generator=g), 'ref_img': torch.rand(2, 3, S, S, generator=g), 'txt_emb': torch.randn(2, 77, 64, generator=g)}
    x_T = torch.randn(2, 4, 8, 8, generator=g)
    got = model.log_results(dict(batch), 0, x_T=x_T)
    seg = model.parse_images(batch['src_img'].to(DEV))
    want = model.log_results({**batch, 'nonmakeup_seg': seg}, 0, x_T=x_T)
    for k in ('samples', 'samples_cfg_scale_9.00', 'mask_pixel'):
        assert torch.equal(got[k], want[k]), k


def test_runs_test_py_with_a_random_face_parser(tmp_path):
    """runs/test.py --face-parser random --paste-background in a fresh child process: no label maps on disk, none synthesised"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(root, 'runs', 'test.py'), '--pairs', '1', '--res', '64', '--batch-size', '1', '--ddim-steps', '2',
                        '--seed', '7', '--out', str(out), '--face-parser', 'random', '--paste-background'],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'mask_pixel' in r.stdout and any(n.startswith('latents_') for n in os.listdir(out))


def test_find_boxes_on_the_device():
    """find_boxes with its two device calls (mkd_crop_resize of the whole photo, the box of mkd_region_mask_from_labels) on a parser
    stand-in that returns a known blob: the box the host arithmetic gives for the blob's extent, and ValueError for an empty map"""
    from makeupdiffuse_amd import photo
    S, H, W = 64, 300, 200
    lab = torch.zeros(1, S, S, dtype=torch.uint8)
    lab[0, 20:32, 20:32] = 1; lab[0, 24, 25] = 7; lab[0, 0, 0] = 8          # skin with a lip pixel; an ear pixel is no face class

    class Blob:
        def __init__(self, maps): self.maps = maps
        def parse(self, img01, out_size=None, lut=None):
            assert tuple(img01.shape) == (self.maps.shape[0], 3, S, S) and img01.device.type == 'cuda'
            return self.maps.to(DEV)

    photo_t = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    (box,) = fp.find_boxes(Blob(lab), [photo_t], grow=1.0, parse_size=S)
    scaled = (20 * H // S, -(-32 * H // S) - 1, 20 * W // S, -(-32 * W // S) - 1)
    assert box == photo.grow_square_box(scaled, H, W, 1.0)
    with pytest.raises(ValueError, match='photo 1'):
        fp.find_boxes(Blob(torch.cat([lab, torch.zeros_like(lab)])), [photo_t, photo_t], parse_size=S)
