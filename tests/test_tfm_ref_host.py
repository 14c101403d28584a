"""No GPU: the float64 references of tests/tfm_ref.py agree with the plain fp32 chains, and the inputs of tests/test_gpu_tfm_tail.py
satisfy the conditions their tests rely on (designated-key weight, key coverage, score levels, row-norm floor)."""
import pytest
import torch
import torch.nn.functional as F

from tests import tfm_ref as R

D = 320
TKS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 77, 79, 80]


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize('B,T,Tk', [(1, 64, 77), (2, 128, 16), (2, 64, 1)])
def test_tail_ref_without_rounding_is_the_fp32_chain(B, T, Tk):
    w = R.block_weights(D, seed=3 + Tk)
    a1, h0, xin, kv = R.random_inputs(B, T, Tk, D, 8, seed=5)
    ref = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D, mirror=False)
    chain = R.torch_chain(w, a1[:, :D], h0[:, :D], xin[:, :D], kv, B, T, Tk, D)
    assert rel(chain, ref) <= 1e-5
    # the storage roundings move the result by a few bf16 steps, not more
    mir = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D)
    assert torch.equal(mir, R.q16(mir.float()).double())
    assert 1e-4 <= rel(mir, ref) <= 6e-3


def test_head_ref_without_rounding_is_the_fp32_chain():
    B, T = 3, 192
    w = R.head_weights(D, seed=2)
    x = R.head_inputs(B, T, D, 8, seed=4)
    h0, qkv = R.head_ref(w, x, B, T, D, mirror=False)
    xf = x[:, :D].view(B, T, D).permute(0, 2, 1)
    gn = F.group_norm(xf, 32, w['gn_g'], w['gn_b'], 1e-6).permute(0, 2, 1).reshape(B * T, D)
    h0c = gn @ w['pi_w'].T + w['pi_b']
    ln = F.layer_norm(h0c, (D,), w['n1_g'], w['n1_b'], 1e-5)
    qkvc = torch.cat([ln @ w['q_w'].T, ln @ w['k_w'].T, ln @ w['v_w'].T], 1)
    assert rel(h0c, h0) <= 1e-5 and rel(qkvc, qkv) <= 1e-5
    h0m, qkvm = R.head_ref(w, x, B, T, D)
    assert rel(h0m, h0) <= 4e-3 and rel(qkvm, qkv) <= 6e-3
    # the second stage alone, from a stored h0
    assert torch.equal(R.head_ref(w, None, B, T, D, h0=h0m)[1], qkvm)
    # the samples' GroupNorm statistics differ by design
    m = x[:, :D].view(B, T, 32, D // 32).mean((1, 3))
    assert (m[1] - m[0]).abs().min() > 0.5 and (m[2] - m[1]).abs().min() > 0.5


@pytest.mark.parametrize('Tk', TKS)
def test_spiked_context_every_key_is_designated_with_nearly_all_the_weight(Tk):
    B, T = 2, 128
    w = R.weights_x(D, seed=11)
    a1, h0, xin, kv, des = R.spiked_inputs(B, T, Tk, D, 0, seed=100 + Tk)
    parts = {}
    ref = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D, parts=parts)
    pw = parts['probs'].gather(-1, des.unsqueeze(-1)).squeeze(-1)               # [B, heads, T]
    assert pw.min() >= 0.95, pw.min()
    for b in range(B):
        for h in range(R.HEADS):
            assert des[b, h].unique().numel() == Tk
    assert not torch.equal(kv[:Tk, D:], kv[Tk:, D:])                            # V differs per sample
    R.row_err(ref, ref)                                                         # the row-norm floor
    # out = h0 + a2 and a2 is the designated V row
    assert rel(ref, R.tail_ref(w, torch.zeros_like(a1), h0, xin, kv, B, T, Tk, D)) == 0.0
    if Tk == 77:      # the seeded error the construction is for: without the last key, the rows that designate it move by tens of percent
        kv2 = kv.view(B, Tk, 2 * D)[:, :Tk - 1].reshape(B * (Tk - 1), 2 * D)
        e = R.row_err(R.tail_ref(w, a1, h0, xin, kv2, B, T, Tk - 1, D), ref)
        # (at least one token per (sample, head) designates it, each in a row of its own)
        assert (e > 0.05).sum() >= B * R.HEADS and e.max() > 0.3, ((e > 0.05).sum(), e.max())


@pytest.mark.parametrize('Tk', [77, 80])
@pytest.mark.parametrize('hard', [False, True])
def test_soft_scores_have_std_about_four(Tk, hard):
    B, T = 2, 128
    w = R.weights_x(D, seed=12)
    a1, h0, xin, kv = R.soft_inputs(B, T, Tk, D, 0, seed=200 + Tk, hard=hard)
    parts = {}
    ref = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D, parts=parts)
    q = parts['q'].view(B, T, R.HEADS, D // R.HEADS).permute(0, 2, 1, 3)
    k = kv[:, :D].double().view(B, Tk, R.HEADS, D // R.HEADS).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * (D // R.HEADS) ** -0.5
    if hard:
        keep = (R.hard_rows(B * T, D, 200 + Tk + 1, zero_row=False)[1] != 4).view(B, 1, T, 1).expand_as(s)
        s = s[keep]                      # (constant rows: LayerNorm output 0, scores 0)
    assert 3.0 <= s.std().item() <= 5.0
    R.row_err(ref, ref)


@pytest.mark.parametrize('Tk', [1, 17, 79])
def test_padding_variant_real_scores_lose_to_a_zero_key(Tk):
    B, T = 2, 128
    w = R.weights_x(D, seed=13, norm2_b=1.0)
    a1, h0, xin, kv = R.padding_inputs(B, T, Tk, D, 0, seed=300 + Tk)
    parts = {}
    ref = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D, parts=parts)
    q = parts['q'].view(B * T, R.HEADS, D // R.HEADS)
    s = -3.0 * q.sum(-1) * (D // R.HEADS) ** -0.5                               # the score of every real key
    assert s.max() <= -8.0 and abs(s.mean().item() + 19.0) <= 1.0, (s.max(), s.mean())
    # one unmasked padded key (score 0, V = 0) would take >= 1 - 80 e^-8 of the weight and pull a2 to 0
    R.row_err(ref, ref)
    assert (ref - h0[:, :D].double()).norm(dim=1).min() > 0.05 * ref.norm(dim=1).median()


@pytest.mark.parametrize('hard', [False, True])
def test_feed_forward_set_cancels_the_residual(hard):
    B, T, Tk = 2, 128, 77
    w = R.weights_f(D, seed=14)
    a1, h0, xin, kv = R.ff_inputs(B, T, Tk, D, 0, seed=400, hard=hard)
    parts = {}
    ref = R.tail_ref(w, a1, h0, xin, kv, B, T, Tk, D, parts=parts)
    assert torch.equal(parts['h2'], h0[:, :D].double())                         # h1 = h2 = h0 exactly
    assert torch.equal(R.q16(-h0), -h0)
    R.row_err(ref, ref)                                                  # incl. the rows with offset 100 and the constant ones
    ff = R.tail_ref(w, a1, h0, torch.zeros_like(xin), kv, B, T, Tk, D, mirror=False) - h0[:, :D].double()
    assert rel(ref, ff) <= 6e-3
    if hard:
        hr, cls = R.hard_rows(B * T, D, 401)
        assert torch.equal(hr, h0[:, :D])
        assert (cls == 4).sum() == 16
        for c, (off, std) in enumerate(R.HARD_LEVELS, 1):
            rows = hr[cls == c]
            assert abs(rows.mean().item() - off) < 0.1 * abs(off) and abs(rows.std(dim=1).mean().item() / std - 1) < 0.2
        assert (hr[16:32].std(dim=1) == 0).all() and (hr[16] == 0).all()
        # every 16-token fragment but the constant one interleaves hard and ordinary rows
        frag = cls.view(-1, 16)
        assert all((f == 0).any() and (f == 2).any() for i, f in enumerate(frag) if i != 1)


def test_head_hard_group_has_mean_fifty_std():
    B, T = 3, 192
    x = R.head_inputs(B, T, D, 0, seed=6, hard_group=5)[:, :D].view(B, T, 32, D // 32)
    m, s = x.mean((1, 3)), x.std((1, 3))
    assert ((m[:, 5] / s[:, 5]) > 25).all() and ((m / s).abs()[:, :5] < 3).all()
    w = R.head_weights(D, seed=7, pi_b=30.0)
    h0, qkv = R.head_ref(w, R.head_inputs(B, T, D, 0, seed=6), B, T, D)
    assert (h0.mean(1) / h0.std(1)).min() > 10
    R.row_err(h0, h0); R.row_err(qkv, qkv)
