"""The fused transformer tail / head (csrc/kernels_tfm.hip) three ways, parametrised by the block width d:

  * tail_ref / head_ref: float64 torch on the CPU, the same operation as the kernels (UPSTREAM cldm BasicTransformerBlock +
    SpatialTransformer.proj_in / proj_out), rounding to bf16 exactly where the kernels STORE bf16 - tail: h1, q,
    a2, h2, the GEGLU intermediate, out; head: the GroupNorm output, h0, q | k | v.  On rows with a large common offset the bf16
    spacing of h1 / h2 is a visible fraction of the row's std: a reference that does not round there measures the storage format,
    not the kernel.  mirror=False turns the rounding off (then tail_ref is torch_chain in float64).
  * tail_unfused / head_unfused: the same block on the GPU as a chain of single kernels the suite tests one by one, through the C
    ABI (mkd_gemm_bf16, mkd_fold_layernorm + mkd_gemm_ln_bf16 incl. the interleaved GEGLU fold, mkd_attention, mkd_groupnorm).  This
    is the yardstick of the per-row tolerances, not the code under test.
  * the input constructors of tests/test_gpu_tfm_tail.py, whose own conditions tests/test_tfm_ref_host.py asserts without a GPU.

Everything a constructor returns is fp32 on the CPU holding bf16-exact values (activations) or plain fp32 (weights)."""
import math

import torch
import torch.nn.functional as F

HEADS = 8
ORDER = ['to_out1_w', 'to_out1_b', 'norm2_g', 'norm2_b', 'to_q2_w', 'to_out2_w', 'to_out2_b', 'norm3_g', 'norm3_b', 'ff0_w', 'ff0_b',
         'ff2_w', 'ff2_b', 'proj_out_w', 'proj_out_b']
HEAD_ORDER = ['gn_g', 'gn_b', 'pi_w', 'pi_b', 'n1_g', 'n1_b', 'q_w', 'k_w', 'v_w']
# (offset, std) of the hard LayerNorm rows: the ADVICE r2 levels of test_gemm_layernorm_on_the_fly_rows_with_mean_far_above_std
HARD_LEVELS = [(50.0, 0.5), (100.0, 1.0), (-30.0, 0.25)]


def q16(t):
    """fp32 -> the nearest bf16, kept as fp32."""
    return t.to(torch.bfloat16).float()


def _rb(x, on):
    return x.to(torch.bfloat16).double() if on else x


def _f64(t, d=None):
    t = t.detach().float().cpu().double()
    return t if d is None else t[:, :d]


def _ln(x, g, b, eps=1e-5):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * g + b


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


# ---- references -------------------------------------------------------------------------------------------------------------
def torch_chain(w, a1, h0, xin, kv, B, T, Tk, d, heads=HEADS):
    """fp32 reference on the bf16-rounded INPUTS (a1, h0, x_in, K | V); weights fp32 as given."""
    dh = d // heads
    h1 = a1 @ w['to_out1_w'].T + w['to_out1_b'] + h0
    q = F.layer_norm(h1, (d,), w['norm2_g'], w['norm2_b'], 1e-5) @ w['to_q2_w'].T
    k = kv[:, :d].reshape(B, Tk, heads, dh).permute(0, 2, 1, 3)
    v = kv[:, d:].reshape(B, Tk, heads, dh).permute(0, 2, 1, 3)
    qh = q.reshape(B, T, heads, dh).permute(0, 2, 1, 3)
    att = torch.softmax(qh @ k.transpose(-1, -2) * dh ** -0.5, dim=-1) @ v
    a2 = att.permute(0, 2, 1, 3).reshape(B * T, d)
    h2 = a2 @ w['to_out2_w'].T + w['to_out2_b'] + h1
    u = F.layer_norm(h2, (d,), w['norm3_g'], w['norm3_b'], 1e-5) @ w['ff0_w'].T + w['ff0_b']
    gg = u[:, :4 * d] * F.gelu(u[:, 4 * d:])
    h3 = gg @ w['ff2_w'].T + w['ff2_b'] + h2
    return h3 @ w['proj_out_w'].T + w['proj_out_b'] + xin


def tail_ref(w, a1, h0, xin, kv, B, T, Tk, d, heads=HEADS, mirror=True, parts=None):
    """float64 tail; a1 / h0 / xin [B*T, >= d], kv [B*Tk, 2d] (any device / dtype).  parts: a dict that receives the
    intermediates (h1, q, probs [B, heads, T, Tk], a2, h2, gg)."""
    dh = d // heads
    W = {k: w[k].detach().cpu().double() for k in ORDER}
    a1, h0, xin, kv = _f64(a1, d), _f64(h0, d), _f64(xin, d), _f64(kv)
    h1 = _rb(a1 @ W['to_out1_w'].T + W['to_out1_b'] + h0, mirror)
    q = _rb(_ln(h1, W['norm2_g'], W['norm2_b']) @ W['to_q2_w'].T, mirror)
    k = kv[:, :d].reshape(B, Tk, heads, dh).permute(0, 2, 1, 3)
    v = kv[:, d:].reshape(B, Tk, heads, dh).permute(0, 2, 1, 3)
    qh = q.reshape(B, T, heads, dh).permute(0, 2, 1, 3)
    probs = torch.softmax(qh @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
    a2 = _rb((probs @ v).permute(0, 2, 1, 3).reshape(B * T, d), mirror)
    h2 = _rb(a2 @ W['to_out2_w'].T + W['to_out2_b'] + h1, mirror)
    u = _ln(h2, W['norm3_g'], W['norm3_b']) @ W['ff0_w'].T + W['ff0_b']
    gg = _rb(u[:, :4 * d] * _gelu(u[:, 4 * d:]), mirror)
    h3 = gg @ W['ff2_w'].T + W['ff2_b'] + h2                     # (never stored: the kernel folds ff.net.2 into proj_out)
    out = _rb(h3 @ W['proj_out_w'].T + W['proj_out_b'] + xin, mirror)
    if parts is not None:
        parts.update(h1=h1, q=q, probs=probs, a2=a2, h2=h2, gg=gg)
    return out


def head_ref(w, x, B, T, d, eps=1e-6, mirror=True, h0=None):
    """float64 head: GroupNorm(32, eps) -> proj_in -> LayerNorm 1 -> to_q | to_k | to_v.  Returns (h0, qkv).  h0 given: q | k | v
    of THAT stored h0 (the second stage alone: on rows with a large common offset one bf16 step of h0 is a visible fraction of the
    row's std, so a chain from x would measure where the producer's rounding fell)."""
    W = {k: w[k].detach().cpu().double() for k in HEAD_ORDER}
    if h0 is None:
        xf = _f64(x, d).view(B, T, d)
        xg = xf.view(B, T, 32, d // 32)
        m = xg.mean((1, 3), keepdim=True)
        v = ((xg - m) ** 2).mean((1, 3), keepdim=True)
        gn = _rb((((xg - m) / torch.sqrt(v + eps)).view(B, T, d) * W['gn_g'] + W['gn_b']).reshape(B * T, d), mirror)
        h0 = _rb(gn @ W['pi_w'].T + W['pi_b'], mirror)
    else:
        h0 = _f64(h0, d)
    ln = _ln(h0, W['n1_g'], W['n1_b'])
    qkv = _rb(torch.cat([ln @ W['q_w'].T, ln @ W['k_w'].T, ln @ W['v_w'].T], 1), mirror)
    return h0, qkv


def row_err(out, ref, d=None):
    """per token ||out_r - ref_r|| / ||ref_r||; asserts that no reference row is small enough to need leaving out."""
    out, ref = _f64(out, d), _f64(ref, d)
    assert torch.isfinite(out).all(), 'non-finite output'
    n = ref.norm(dim=1)
    assert n.min() >= 0.25 * n.median(), f'reference row norm {n.min():.3e} < 0.25 x median {n.median():.3e}'
    return (out - ref).norm(dim=1) / n


# ---- the unfused chains (GPU, C ABI) -------------------------------------------------------------------------------------------
def _gpu():
    from tests import gpu_util
    return gpu_util


def _gemm(A, lda, W, bias, R, ldr, M, N, K):
    u = _gpu()
    out = torch.empty(M, N, device=u.DEV, dtype=torch.bfloat16)
    rc = u.L().mkd_gemm_bf16(u.P(A), lda, u.P(W), K, u.P(bias), None, 0, 1, u.P(R), ldr, 1.0, 0, u.P(out), N, 0, M, N, K,
                             0, 0, 0, 0, 0, 0, 0, 1, 0, 0, None)
    assert rc == 0, u.L().mkd_last_error()
    return out


def _fold(W, gamma, beta, bias, geglu=False):
    """mkd_fold_layernorm of fp32 device W [N, K]: (W' bf16, s, b'); geglu: rows [0, N/2) value, [N/2, N) gate, interleaved."""
    u = _gpu()
    N, K = W.shape
    Wf = torch.empty(N, K, device=u.DEV, dtype=torch.bfloat16); s = torch.empty(N, device=u.DEV); b = torch.empty(N, device=u.DEV)
    if geglu:
        inner = N // 2
        for half in range(2):
            rc = u.L().mkd_fold_layernorm(u.P(W[half * inner:]), u.P(gamma), u.P(beta), u.P(None if bias is None else bias[half * inner:]),
                                          inner, K, u.P(Wf), half, 2, u.P(s), u.P(b), None)
            assert rc == 0, u.L().mkd_last_error()
    else:
        rc = u.L().mkd_fold_layernorm(u.P(W), u.P(gamma), u.P(beta), u.P(bias), N, K, u.P(Wf), 0, 1, u.P(s), u.P(b), None)
        assert rc == 0, u.L().mkd_last_error()
    return Wf, s, b


def _gemm_ln(A, lda, folded, M, K, act=0):
    u = _gpu()
    Wf, s, b = folded
    N = Wf.shape[0]
    ncol = N // 2 if act == 2 else N
    out = torch.empty(M, ncol, device=u.DEV, dtype=torch.bfloat16)
    rc = u.L().mkd_gemm_ln_bf16(u.P(A), lda, u.P(Wf), K, u.P(b), u.P(s), None, 0, 1e-5, act, u.P(out), ncol, M, N, K, None)
    assert rc == 0, u.L().mkd_last_error()
    return out


def tail_unfused(w, a1, ld, h0, xin, kv, B, T, Tk, d, heads=HEADS):
    """a1 / h0 / xin: bf16 device [B*T, ld]; kv: bf16 device [B*Tk, 2d].  The launches of the engine's unfused plan: to_out1, LN2 . to_q,
    cross-attention, to_out2, LN3 . ff.net.0 + GEGLU, the merged [proj_out . ff.net.2 | proj_out] product on [gg | h2]."""
    u = _gpu()
    M, dh = B * T, d // heads
    dev = {k: w[k].to(u.DEV).float().contiguous() for k in ORDER}
    h1 = _gemm(a1, ld, u.bf(w['to_out1_w']), dev['to_out1_b'], h0, ld, M, d, d)
    q = _gemm_ln(h1, d, _fold(dev['to_q2_w'], dev['norm2_g'], dev['norm2_b'], None), M, d)
    a2 = torch.empty(M, d, device=u.DEV, dtype=torch.bfloat16)
    rc = u.L().mkd_attention(u.P(q), d, u.P(kv), 2 * d, u.P(kv[:, d:]), 2 * d, u.P(a2), d, B, T, Tk, heads, dh, dh ** -0.5, None)
    assert rc == 0, u.L().mkd_last_error()
    h2 = _gemm(a2, d, u.bf(w['to_out2_w']), dev['to_out2_b'], h1, d, M, d, d)
    gg = _gemm_ln(h2, d, _fold(dev['ff0_w'], dev['norm3_g'], dev['norm3_b'], dev['ff0_b'], geglu=True), M, d, act=2)
    Wp, W2 = w['proj_out_w'].double(), w['ff2_w'].double()
    Wm = u.bf(torch.cat([Wp @ W2, Wp], 1).float())
    bm = (Wp @ w['ff2_b'].double() + w['proj_out_b'].double()).float().to(u.DEV)
    out = _gemm(torch.cat([gg, h2], 1).contiguous(), 5 * d, Wm, bm, xin, ld, M, d, 5 * d)
    u.sync()
    return out


def head_unfused(w, x, ld, B, T, d, eps=1e-6):
    """x: bf16 device [B*T, ld].  mkd_groupnorm, proj_in, LN1 . (to_q | to_k | to_v).  Returns (h0, qkv)."""
    u = _gpu()
    M = B * T
    dev = {k: w[k].to(u.DEV).float().contiguous() for k in HEAD_ORDER}
    gn = torch.empty(M, d, device=u.DEV, dtype=torch.bfloat16)
    rc = u.L().mkd_groupnorm(u.P(x), ld, u.P(dev['gn_g']), u.P(dev['gn_b']), eps, 0, u.P(gn), d, B, T, d, 32, None)
    assert rc == 0, u.L().mkd_last_error()
    h0 = _gemm(gn, d, u.bf(w['pi_w']), dev['pi_b'], None, 0, M, d, d)
    Wqkv = torch.cat([dev['q_w'], dev['k_w'], dev['v_w']], 0).contiguous()
    qkv = _gemm_ln(h0, d, _fold(Wqkv, dev['n1_g'], dev['n1_b'], None), M, d)
    u.sync()
    return h0, qkv


# ---- weights ------------------------------------------------------------------------------------------------------------------
def block_weights(d, seed, norm_jitter=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    w = {
        'to_out1_w': r(d, d) / math.sqrt(d), 'to_out1_b': 0.1 * r(d),
        'norm2_g': 1 + norm_jitter * r(d), 'norm2_b': norm_jitter * r(d),
        'to_q2_w': r(d, d) / math.sqrt(d),
        'to_out2_w': r(d, d) / math.sqrt(d), 'to_out2_b': 0.1 * r(d),
        'norm3_g': 1 + norm_jitter * r(d), 'norm3_b': norm_jitter * r(d),
        'ff0_w': r(8 * d, d) / math.sqrt(d), 'ff0_b': 0.1 * r(8 * d),
        'ff2_w': r(d, 4 * d) / math.sqrt(4 * d), 'ff2_b': 0.1 * r(d),
        'proj_out_w': r(d, d) / math.sqrt(d), 'proj_out_b': 0.1 * r(d),
    }
    return w


def weights_x(d, seed, norm2_b=0.0):
    """Set X, cross-attention isolated (every value exactly representable): with x_in = 0, out = h0 + a2(LN(h0) + norm2_b)."""
    w = block_weights(d, seed)
    z, eye = torch.zeros(d), torch.eye(d)
    w.update(to_out1_w=torch.zeros(d, d), to_out1_b=z.clone(), norm2_g=torch.ones(d), norm2_b=torch.full((d,), float(norm2_b)),
             to_q2_w=eye.clone(), to_out2_w=eye.clone(), to_out2_b=z.clone(), ff2_w=torch.zeros(d, 4 * d), ff2_b=z.clone(),
             proj_out_w=eye.clone(), proj_out_b=z.clone())
    return w


def weights_f(d, seed):
    """Set F, feed-forward isolated: with x_in = -h0 the h0 term cancels in the fp32 epilogue, out = ff2(GEGLU(ff0(LN3(h0)))).
    ff2_b is 0.5 randn, so that a constant row (LayerNorm output = norm3_b) keeps a row norm of the order of the others'."""
    w = block_weights(d, seed)
    g = torch.Generator().manual_seed(seed + 99991)
    z = torch.zeros(d)
    w.update(to_out1_w=torch.zeros(d, d), to_out1_b=z.clone(), to_out2_w=torch.zeros(d, d), to_out2_b=z.clone(),
             ff2_b=0.5 * torch.randn(d, generator=g), proj_out_w=torch.eye(d), proj_out_b=z.clone())
    return w


def head_weights(d, seed, pi_b=None, g=None):
    g = g or torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    w = {'gn_g': 1 + 0.2 * r(d), 'gn_b': 0.2 * r(d), 'pi_w': r(d, d) / math.sqrt(d), 'pi_b': 0.1 * r(d), 'n1_g': 1 + 0.2 * r(d), 'n1_b': 0.2 * r(d),
         'q_w': r(d, d) / math.sqrt(d), 'k_w': r(d, d) / math.sqrt(d), 'v_w': r(d, d) / math.sqrt(d)}
    if pi_b is not None:
        w['pi_b'] = w['pi_b'] + pi_b                 # every LayerNorm-1 row gets a large common offset
    return w


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def random_inputs(B, T, Tk, d, pad, seed):
    """activations of the scale the block sees (h0 / x_in: O(1) residual streams with a per-channel offset; a1: attention output)"""
    g = torch.Generator().manual_seed(seed)
    M, ld = B * T, d + pad
    a1 = q16(torch.randn(M, ld, generator=g))
    h0 = q16(torch.randn(M, ld, generator=g) + 0.5 * torch.randn(1, ld, generator=g))
    xin = q16(torch.randn(M, ld, generator=g))
    kv = q16(torch.randn(B * Tk, 2 * d, generator=g))
    return a1, h0, xin, kv


def designated_key(B, T, Tk, heads=HEADS):
    """[B, heads, T]: the context key token t of sample b designates in head h.  Covers every key in every (sample, head) when T >= Tk."""
    t = torch.arange(T).view(1, 1, T); h = torch.arange(heads).view(1, heads, 1); b = torch.arange(B).view(B, 1, 1)
    return (t + 3 * h + 11 * b) % Tk


def spiked_inputs(B, T, Tk, d, pad, seed, heads=HEADS):
    """For set X: every (token, head) puts nearly all its softmax weight on ONE designated key, and every key 0 .. Tk-1 is some
    token's.  h0 = 0.05 randn + one hot channel of +-1 per (token, head); key j = 16 e_(j mod dh), + for j < dh, - for j >= dh; V
    random, different per sample.  x_in = 0; a1 random (to_out1 = 0 must silence it)."""
    g = torch.Generator().manual_seed(seed)
    M, ld, dh = B * T, d + pad, d // heads
    assert Tk <= 2 * dh
    des = designated_key(B, T, Tk, heads)
    h0 = 0.05 * torch.randn(M, ld, generator=g)
    sign = torch.where(des < dh, 1.0, -1.0)                                   # [B, heads, T]
    col = torch.arange(heads).view(1, heads, 1) * dh + des % dh
    rows = (torch.arange(B).view(B, 1, 1) * T + torch.arange(T).view(1, 1, T)).expand(B, heads, T)
    h0[rows.reshape(-1), col.reshape(-1)] += sign.reshape(-1)
    kv = torch.zeros(B * Tk, 2 * d)
    j = torch.arange(Tk)
    for b in range(B):
        for h in range(heads):
            kv[b * Tk + j, h * dh + j % dh] = torch.where(j < dh, 16.0, -16.0)
    kv[:, d:] = torch.randn(B * Tk, d, generator=g)
    a1 = q16(torch.randn(M, ld, generator=g))
    return a1, q16(h0), torch.zeros(M, ld), q16(kv), des


def soft_inputs(B, T, Tk, d, pad, seed, hard=False):
    """For set X: K = 4 randn, so the scores have std ~ 4 (this is where the softmax scale shows).  hard: h0 from hard_rows."""
    a1, h0, xin, kv = random_inputs(B, T, Tk, d, pad, seed)
    g = torch.Generator().manual_seed(seed + 4242)
    kv[:, :d] = q16(4.0 * torch.randn(B * Tk, d, generator=g))
    if hard:
        h0[:, :d] = hard_rows(B * T, d, seed + 1, zero_row=False)[0]
    return a1, h0, torch.zeros_like(xin), kv


def padding_inputs(B, T, Tk, d, pad, seed):
    """For set X with norm2_b = 1: every key is -3 ones, so every real score is ~ -19 and all real keys weigh the same; a zero-padded
    key past Tk would score 0 and, unmasked, take all the weight."""
    a1, h0, xin, kv = random_inputs(B, T, Tk, d, pad, seed)
    kv[:, :d] = -3.0
    return a1, h0, torch.zeros_like(xin), kv


def hard_rows(M, d, seed, zero_row=True):
    """h0 [M, d] for the LayerNorm-statistics sets: rows 1 / 3 / 5 (mod 8) are offset + std randn at the HARD_LEVELS, the others
    ordinary rows, so every 16-token fragment interleaves both; rows 16 .. 31 are constant (std 0; one of them all zero on request).
    Returns (h0, cls): cls 0 ordinary, 1 .. 3 the hard levels, 4 constant."""
    g = torch.Generator().manual_seed(seed)
    h0 = torch.randn(M, d, generator=g) + 0.5 * torch.randn(1, d, generator=g)
    cls = torch.zeros(M, dtype=torch.long)
    for i, (off, std) in enumerate(HARD_LEVELS):
        sel = torch.arange(M) % 8 == 2 * i + 1
        h0[sel] = off + std * torch.randn(int(sel.sum()), d, generator=g)
        cls[sel] = i + 1
    for i in range(16):
        c = (-1.0) ** i * (0.5 + 0.125 * i)
        h0[16 + i] = 0.0 if (zero_row and i == 0) else c
    cls[16:32] = 4
    return q16(h0), cls


def ff_inputs(B, T, Tk, d, pad, seed, hard=False):
    """For set F: x_in = -h0 (exact in bf16)."""
    a1, h0, xin, kv = random_inputs(B, T, Tk, d, pad, seed)
    if hard:
        h0[:, :d] = hard_rows(B * T, d, seed + 1)[0]
    return a1, h0, -h0, kv


def head_inputs(B, T, d, pad, seed, hard_group=None):
    """x [B*T, d + pad]: per-channel scale / offset (the group statistics matter), then per sample a scale b + 1 and an offset b - 1,
    so the samples' GroupNorm statistics differ by design.  hard_group: that group's channels get + 50 (b + 1): mean / std ~ 50."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    ld = d + pad
    x = (r(B * T, ld) * (1 + 0.5 * r(1, ld)) + 0.3 * r(1, ld)).view(B, T, ld)
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    x = x * (b + 1) + (b - 1)
    if hard_group is not None:
        cg = d // 32
        x[:, :, hard_group * cg:(hard_group + 1) * cg] += 50.0 * (b + 1)
    return q16(x.reshape(B * T, ld))
