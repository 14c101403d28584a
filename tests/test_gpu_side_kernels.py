"""-m gpu: the small kernels that only the side networks reach (first-stage decoder and encoder, CLIP embeddings, the time embedding,
the interpolation blend), each through its own C-ABI entry against float64 on the same rounded inputs, element by element.

fp32 results of a length-n dot product are held to the a-priori bound of gpu_util.dot_bound, (n + 16) 2^-24 sum |a_i b_i|: it needs
no measuring, and a missed tap, lane or channel exceeds it by orders of magnitude.  (The conv3x3_direct arms of the side networks are
in tests/test_gpu_kernels.py, next to the cases that were there.)"""
import math

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, L, P, assert_within, bf, dot_bound, sync

pytestmark = pytest.mark.gpu


# ---- softmax_rows: fp32 scores in (what the mid attention feeds it), bf16 probabilities out ---------------------------------------------
def softmax_rows_input(cols):
    k = torch.arange(cols, dtype=torch.float32)
    g = torch.Generator().manual_seed(cols)
    equal = torch.full((cols,), 3.25)
    peak = torch.randn(cols, generator=g); peak[cols // 3] = peak.max() + 60.0
    tied = torch.randn(cols, generator=g).clamp(max=1.0); tied[0] = 2.0; tied[cols - 1] = 2.0
    ramp = -0.5 * k
    low = torch.full((cols,), -1e4)
    return torch.stack([equal, peak, tied, ramp, low, torch.randn(cols, generator=g) * 9])


@pytest.mark.parametrize('cols', [1, 48, 256, 300, 1024])
def test_softmax_rows(cols):
    x = softmax_rows_input(cols).to(DEV)
    rows = x.shape[0]
    y = torch.full((rows, cols), float('nan'), device=DEV, dtype=torch.bfloat16)
    assert L().mkd_softmax_rows(P(x), P(y), rows, cols, None) == 0, L().mkd_last_error()
    sync()
    ref = torch.softmax(x.double().cpu(), -1)
    # bf16 rounding of p is 2^-9 p; the rest of 2^-8 p is for exp and the row sum in fp32
    assert_within(y, ref, 2.0 ** -8 * ref + 1e-7, f'softmax_rows cols {cols}')
    sums = y.double().cpu().sum(-1)
    assert ((sums - 1).abs() <= 2.0 ** -8).all(), f'softmax_rows cols {cols}: row sums {sums.tolist()}'


# ---- vae_enc_tail: conv_out -> quant_conv -> moments, posterior sample --------------------------------------------------------------------
def enc_tail_problem(B, H, W_, Cin):
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W_ * 10 + Cin)
    x = bf(torch.randn(B, H, W_, Cin, generator=g))
    w = bf(torch.randn(8, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    bias = (0.1 * torch.randn(8, generator=g)).to(DEV)
    wq = bf(torch.randn(8, 8, generator=g) / math.sqrt(8))
    bq = 0.1 * torch.randn(8, generator=g)
    bq[4:8] = torch.tensor([-40.0, -5.0, 10.0, 30.0])          # log-variance below -30, inside, inside, above 20: both clamps engage
    noise = torch.randn(B, 4, H, W_, generator=g).to(DEV)
    wp = torch.empty(8, 9 * Cin, device=DEV, dtype=torch.bfloat16)
    assert L().mkd_pack_conv_weight(P(w.float().contiguous()), P(wp), 8, Cin, 3, 3, None) == 0
    return x, w, wp, bias, wq, bq.to(DEV), noise


def enc_tail(x, wp, bias, wq, bq, noise, scale, want_z=True, want_mom=True):
    B, H, W_, Cin = x.shape
    z = torch.full((B, 4, H, W_), float('nan'), device=DEV) if want_z else None
    mom = torch.full((B, 8, H, W_), float('nan'), device=DEV) if want_mom else None
    rc = L().mkd_vae_enc_tail(P(x), P(wp), P(bias), P(wq), P(bq), P(noise), scale, P(z), P(mom), B, H, W_, Cin, 4, None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return z, mom


@pytest.mark.parametrize('B,H,W_,Cin', [(1, 5, 7, 64), (2, 4, 4, 512), (3, 3, 3, 8)])
def test_vae_enc_tail(B, H, W_, Cin):
    x, w, wp, bias, wq, bq, noise = enc_tail_problem(B, H, W_, Cin)
    scale = 0.18215
    z, mom = enc_tail(x, wp, bias, wq, bq, noise, scale)
    # moments: the dot-product bound of conv_out, carried through quant_conv, plus quant_conv's own
    xd = x.double().cpu().permute(0, 3, 1, 2); wd = w.double().cpu(); bd = bias.double().cpu()
    wqd = wq.double().cpu(); bqd = bq.double().cpu()
    acc = F.conv2d(xd, wd, bd, padding=1)
    e_acc = dot_bound(9 * Cin + 1, F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1))
    ref = torch.einsum('oi,bihw->bohw', wqd, acc) + bqd[None, :, None, None]
    bound = torch.einsum('oi,bihw->bohw', wqd.abs(), e_acc) + \
        dot_bound(8 + 1, torch.einsum('oi,bihw->bohw', wqd.abs(), acc.abs()) + bqd.abs()[None, :, None, None])
    assert_within(mom, ref, bound, f'enc_tail moments {B}x{H}x{W_}x{Cin}')
    lv = ref[:, 4:]
    assert (lv[:, 0] < -30).all() and (lv[:, 3] > 20).all() and (lv[:, 1:3].abs() < 20).all()
    # z from the device's OWN moments: exact up to fp32 rounding of exp
    md = mom.double().cpu()

    def latent(nz):
        std = torch.exp(0.5 * md[:, 4:].clamp(-30.0, 20.0))
        return (md[:, :4] + (std * nz.double().cpu() if nz is not None else 0.0)) * float(torch.tensor(scale, dtype=torch.float32))
    torch.testing.assert_close(z.double().cpu(), latent(noise), rtol=1e-5, atol=1e-5)
    z_mode, mom2 = enc_tail(x, wp, bias, wq, bq, None, scale)
    assert torch.equal(mom2, mom)
    torch.testing.assert_close(z_mode.double().cpu(), latent(None), rtol=1e-5, atol=1e-5)
    # either output may be left out; the other keeps its bits
    z_only, none = enc_tail(x, wp, bias, wq, bq, noise, scale, want_mom=False)
    assert none is None and torch.equal(z_only, z)
    none, mom_only = enc_tail(x, wp, bias, wq, bq, noise, scale, want_z=False)
    assert none is None and torch.equal(mom_only, mom)


def test_vae_enc_tail_refuses_bad_arguments():
    x, w, wp, bias, wq, bq, noise = enc_tail_problem(1, 2, 2, 8)
    lib = L()
    z = torch.zeros(1, 4, 2, 2, device=DEV)
    assert lib.mkd_vae_enc_tail(P(x), P(wp), P(bias), P(wq), P(bq), None, 1.0, None, None, 1, 2, 2, 8, 4, None) == -1
    assert lib.mkd_vae_enc_tail(P(x), P(wp), P(bias), P(wq), P(bq), None, 1.0, P(z), None, 1, 2, 2, 8, 8, None) == -1
    assert lib.mkd_vae_enc_tail(P(x), P(wp), P(bias), P(wq), P(bq), None, 1.0, P(z), None, 1, 2, 2, 12, 4, None) == -1


# ---- post_quant: 1x1 conv over fp32 NCHW latents with 1 / scale_factor folded in ------------------------------------------------------
@pytest.mark.parametrize('B,C_,hw', [(2, 4, 35), (1, 4, 1024)])
def test_post_quant(B, C_, hw):
    g = torch.Generator().manual_seed(hw)
    z = (torch.randn(B, C_, hw, generator=g) * 0.18215).to(DEV)
    w = bf(torch.randn(C_, C_, generator=g) / math.sqrt(C_))
    bias = (0.1 * torch.randn(C_, generator=g)).to(DEV)
    inv = torch.tensor(1.0 / 0.18215, dtype=torch.float32)
    out = torch.full((B, C_, hw), float('nan'), device=DEV)
    assert L().mkd_post_quant(P(z), P(w), P(bias), float(inv), P(out), B, C_, hw, None) == 0, L().mkd_last_error()
    sync()
    zs = z.double().cpu() * inv.double()
    wd, bd = w.double().cpu(), bias.double().cpu()
    ref = torch.einsum('oi,bip->bop', wd, zs) + bd[None, :, None]
    bound = dot_bound(C_ + 1, torch.einsum('oi,bip->bop', wd.abs(), zs.abs()) + bd.abs()[None, :, None])
    assert_within(out, ref, bound, f'post_quant {B}x{C_}x{hw}')


# ---- timestep_embedding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [64, 320])
def test_timestep_embedding(dim):
    ts = [0, 1, 37, 500, 999]
    t = torch.tensor(ts, dtype=torch.int64, device=DEV)
    out = torch.full((len(ts), dim), float('nan'), device=DEV, dtype=torch.bfloat16)
    assert L().mkd_timestep_embedding(P(t), P(out), len(ts), dim, None) == 0, L().mkd_last_error()
    sync()
    half = dim // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = torch.tensor(ts, dtype=torch.float64)[:, None] * freq[None]
    ref = torch.cat([torch.cos(a), torch.sin(a)], -1)
    # 2^-9: bf16 rounding in [-1, 1]; 3e-4: the fp32 argument t f_k at up to 999 rad (half an ulp of 999 is 3e-5, f_k itself carries a
    # few 1e-7 relative from expf)
    assert_within(out, ref, torch.full_like(ref, 2.0 ** -9 + 3e-4), f'timestep_embedding dim {dim}')
    assert out[0, :half].float().eq(1).all() and out[0, half:].float().eq(0).all()          # t = 0: cos 1, sin 0 exactly


# ---- clip_embed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,width,vocab', [(2, 77, 768, 1000), (3, 5, 64, 50)])
def test_clip_embed(B, T, width, vocab):
    g = torch.Generator().manual_seed(width)
    tok = bf(torch.randn(vocab, width, generator=g))
    pos = bf(torch.randn(T, width, generator=g))
    ids = torch.randint(0, vocab, (B, T), generator=g, dtype=torch.int32)
    ids[0, 0] = 0; ids[0, 1] = vocab - 1; ids[-1, -1] = vocab - 1; ids[-1, 0] = 0
    ids[0, 2] = ids[0, 3] = ids[1, 2] = 7                       # repeats, in one sample and across samples
    ids = ids.to(DEV)
    out = torch.full((B, T, width), float('nan'), device=DEV, dtype=torch.bfloat16)
    assert L().mkd_clip_embed(P(ids), P(tok), P(pos), P(out), B, T, width, vocab, None) == 0, L().mkd_last_error()
    sync()
    want = (tok.float()[ids.long()] + pos.float()[None]).bfloat16()
    assert torch.equal(out, want)


# ---- blend_bf16 ------------------------------------------------------------------------------------------------------------------
def test_blend_bf16():
    batch, per = 3, 8 * 37                                        # 111 vectors of 8: the sample borders fall inside one thread block
    g = torch.Generator().manual_seed(5)
    a = bf(torch.randn(batch, per, generator=g) * 3)
    b = bf(torch.randn(batch, per, generator=g) * 3)
    alpha = torch.tensor([0.0, 1.0, 0.3], dtype=torch.float32)
    alpha_d = alpha.to(DEV)
    y = torch.full((batch, per), float('nan'), device=DEV, dtype=torch.bfloat16)
    assert L().mkd_blend_bf16(P(a), P(b), P(alpha_d), P(y), per, batch, None) == 0, L().mkd_last_error()
    sync()
    assert torch.equal(y[0], a[0]) and torch.equal(y[1], b[1])
    al = alpha.double()[:, None]
    ad, bd = a.double().cpu(), b.double().cpu()
    assert_within(y, (1 - al) * ad + al * bd, 2.0 ** -8 * torch.maximum(ad.abs(), bd.abs()), 'blend_bf16')
    assert L().mkd_blend_bf16(P(a), P(b), P(alpha_d), P(y), per - 4, batch, None) == -1
