"""CPU side of tests/test_gpu_gemm_elements.py: the float64 reference of the implicit-GEMM family (csrc/kernels_gemm.hip, kernels_conv.hip)

    C = act(((sum_k A W + bias + rowbias[m // rpb]) scale) + R)

on inputs that are bf16 values already - linear rows, the 3x3 gather (stride 1 | 2, nearest x2 upsampling, pad origin 1), the down conv
(pad bottom / right only, stride 2), the folded second input (3x3 conv + 1x1 of x2) and the GEGLU epilogue on interleaved (value, gate)
rows - with, per output element, the value y and the absolute-value sum S = (sum_k |A||W| + |bias| + |rowbias|) |scale| + |R|; the
per-element bound; the input sets; the cases (the smallest shapes at which each path can still go wrong); the rows of the tile table;
an fp32 emulation of the kernels (64-wide K-steps, split-K slabs, the epilogue in the kernel's order, one rounding) and nine that
are wrong on purpose (tests/test_gemm_ref_host.py shows that the checks separate them).  No GPU, no library call.

The bound, per element, u = 2^-23 (derived, not measured):
    bf16 output, act 0 (none) or 4 (ReLU)     |out - y| <= 2^-8 |y| + (K + 4) u S
        2^-8 |y|       one round-to-nearest to 8 significant bits (half a unit in the last place is at most 2^-8 |y|)
        (K + 4) u S    fp32 accumulation of K exact bf16 x bf16 products in ANY order (K - 1 additions) and the epilogue's four
                       operations (+ bias, + rowbias, x scale, + R), each within u of its result, every partial result within S.
                       u is 2^-23, not the 2^-24 of round-to-nearest, so that the bound also holds if the matrix cores truncate their
                       internal additions: nobody has measured that on this hardware.  The same factor of two covers the
                       (1 + 2^-8) by which the rounding term grows when it is taken of the perturbed value.  ReLU is 1-Lipschitz.
    fp32 output                               |out - y| <= (K + 4) u S
    SiLU (act 1), quick-GELU (act 3)          f(z) = z sigma(k z), k = 1 | 1.702;  |f'| <= 1.0998 < LIP_SILU = 1.1 for both (the maximum
                       of sigma(t)(1 + t (1 - sigma(t))), at t = 2.3994).  sigmoid_scaled_f (mkd_common.h) is rcp(1 + exp2(z c)), c = -k log2 e:
                       the exponent carries two roundings (c, z c), |z c| 2^-23, which exp2 turns into a RELATIVE error of
                       ln 2 |z c| 2^-23 = |k z| 2^-23; exp2 and rcp are within about 1 ulp (2^-23 each), 1 + e and the product with z
                       within 2^-24 each; d ln sigma / d ln e lies in (-1, 0).  So
                           |out - y| <= 2^-8 |y| + 1.1 (K + 4) u S + |y| (|k z| + 3) u
    GEGLU (act 2)     out = a G(g), G(g) = g / 2 (1 + erf(g / sqrt 2)), |G'| <= 1.129 < LIP_GELU = 1.13 (at g = sqrt 2), value a and gate g
                       with their own bounds e_a, e_g = (K + 4) u S_a, S_g.  gelu_erf_f is Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7,
                       evaluated in 16 fp32 operations on values below 2 (32 u in all), so dG = |g| / 2 (1.5e-7 + 32 u) + |G| u:
                           |out - y| <= 2^-8 |y| + |G(g)| e_a + (|a| + e_a)(1.13 e_g + dG) + |y| u
    Every bound also carries 2^-126: a result below the normal range may be flushed to zero.
On the CPU the correct emulation stays within the bound on every case and set below (test_gemm_ref_host.py re-establishes it).  On the
bf16 cases the worst element is always one that the final rounding moves by nearly half a unit in the last place: a value just above a
power of two, where half a unit is nearly 2^-8 |y| - 0.99 of the bound at K = 8 and K = 72 (the fp32 term is then almost nothing), 0.97
at most from K = 136 on, 0.78 at K = 1344.  With fp32 output the emulation reaches 0.003 of the bound: the fp32 term is wide, as
any-order bounds are, and it is the exact set, not this term, that sees a single missing product."""
import math
import os
import re
from collections import namedtuple

import torch

U = 2.0 ** -23
RND = 2.0 ** -8
TINY = 2.0 ** -126
LIP_SILU = 1.1
LIP_GELU = 1.13
ERF_ERR = 1.5e-7 + 32 * U
BK = 64
SETS = ('randn', 'exact', 'ones')
MUTANTS = ('drop_product', 'drop_chunk', 'zero_tap', 'halo_neighbour', 'truncate', 'residual_after_round', 'rowbias_of_wave', 'skip_bias_tail', 'drop_last_slab')
WAVE_ROWS = 32          # rows of a wave in most rows of the table (the row-bias mutant)


def q16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def is_bf16(t):
    return bool(torch.equal(q16(t), t))


# ---- the tile table: one Row per MKD_TILE line of csrc/gemm_tiles.inc -------------------------------------------------------------------
Row = namedtuple('Row', 'index name family TM TN WM WN STAGES KW base')
GATHER_FAMILIES = ('GEMM', 'KSPLIT', 'LIGHT', 'RA')          # gemm_kernel / gemm_ra_kernel: linear rows and the 3x3 gather
_TILE_LINE = re.compile(r'^MKD_TILE\(\s*(\d+),\s*(\w+),\s*(\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)', re.M)


def tile_rows(table=None):
    """The rows of gemm_tiles.inc (wave grid, ring depth, K groups: what mkd_gemm_tile_info does not tell).  table: lib.tile_table(), the
    library's own list [(tile_m, tile_n, lds_staged_conv, name)]: the rows are then the library's, checked one by one."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'makeupdiffuse_amd', 'csrc', 'gemm_tiles.inc')
    with open(path) as f:
        rows = [Row(int(m[1]), m[2], m[3], *(int(m[i]) for i in range(4, 11))) for m in _TILE_LINE.finditer(f.read())]
    assert rows and [r.index for r in rows] == list(range(len(rows)))
    if table is not None:
        assert len(table) == len(rows), f'the library has {len(table)} tile rows, gemm_tiles.inc {len(rows)}: rebuild'
        for r, (tm, tn, patch, name) in zip(rows, table):
            assert (r.TM, r.TN, r.family == 'PATCH', r.name) == (tm, tn, patch, name), f'row {r.index}: {r} != {(tm, tn, patch, name)}'
    return rows


def folds_second_input(row):
    """gemm_cfg_folds_second_input (kernels_gemm.hip): gemm_kernel only."""
    return row.family not in ('PATCH', 'RA')


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# conv: (B, H, W, Cin, Hout, Wout, stride, up, pad_tl, K2) or None;  rpb: rows per row-bias sample (0: no row bias);  splitk: the ABI's
# argument;  lda / ldw: row strides of A (pixel stride) and W;  ldn: stride of R, rowbias and C;  ldx2: row stride of the second input
Conv = namedtuple('Conv', 'B H W Cin Hout Wout stride up pad_tl K2')
Case = namedtuple('Case', 'id kind entry M N K conv bias rpb scale res act f32 splitk lda ldw ldn ldx2')


def _linear(M, N, K, tag='', entry='gemm', bias=True, rpb=0, scale=1.0, res=False, act=0, f32=False, splitk=1, pad=False):
    nout = N // 2 if act == 2 else N
    return Case(f'L{M}x{N}x{K}{tag}', 'linear', entry, M, N, K, None, bias, rpb, scale, res, act, f32, splitk,
                K + 8 if pad else K, K + 8 if pad else K, nout + 4, 0)


def _conv(kind, B, H, W, Cin, Cout, tag='', entry='gemm', stride=1, up=0, pad_tl=1, K2=0, rpb=0, res=False, splitk=1, padx=False):
    if pad_tl == 0:
        Hout, Wout = H // 2, W // 2
    else:
        Hout, Wout = ((H << up) - 1) // stride + 1, ((W << up) - 1) // stride + 1
    K = 9 * Cin + K2
    cid = f'{kind[0].upper()}-B{B}-{H}x{W}-c{Cin}-{Cout}{tag}'
    return Case(cid, kind, entry, B * Hout * Wout, Cout, K, Conv(B, H, W, Cin, Hout, Wout, stride, up, pad_tl, K2), True, rpb, 1.0, res,
                0, False, splitk, Cin + 8 if padx else Cin, K, Cout + 4, K2 + 8 if K2 else 0)


def cases():
    return [
        # linear: K-step counts 1, 2, 3, 6, 8, 21 (and 4 under split-K) against every ring depth and K-group count
        _linear(96, 64, 8),                                                   # one 16-byte chunk of K
        _linear(77, 68, 72),                                                  # a second K-step of one chunk, N ends inside a fragment, ragged tile
        _linear(100, 100, 136, '-silu', act=1),
        _linear(100, 100, 136, '-qgelu', act=3),
        _linear(100, 100, 136, '-f32', f32=True),
        _linear(100, 100, 136, '-relu', act=4, res=True),                     # (ReLU after the residual: the exact set's act 4)
        _linear(300, 132, 456, '-full', rpb=100, scale=0.75, res=True, pad=True),      # samples end inside a tile and inside a wave
        _linear(300, 132, 328),                                               # bias only: the straight-line epilogue
        _linear(520, 320, 1344),
        _linear(130, 324, 200, '-s3-f32', rpb=50, scale=0.75, res=True, f32=True, splitk=3),       # 4 K-steps: 2 slabs of 2
        _linear(130, 324, 200, '-s7-silu', rpb=50, scale=0.75, res=True, act=1, splitk=7),         # clamped to 4 slabs of 1, the last 8 wide
        _linear(100, 136, 136, '-geglu', act=2, splitk=0),
        _linear(100, 136, 136, '-geglu-s2', act=2, splitk=2),
        _linear(300, 132, 456, '-gnstat', entry='gnstat', rpb=100, scale=0.75, res=True, pad=True),
        # 3x3 gather
        _conv('gather', 3, 5, 7, 8, 68),                                      # K = 72: taps change inside a K-step, 35 rows per sample
        _conv('gather', 2, 7, 5, 24, 132, '-s2', stride=2),                   # odd sizes under stride 2 (output 4 x 3)
        _conv('gather', 2, 7, 5, 24, 132, '-s2-split', stride=2, rpb=12, res=True, splitk=3),
        _conv('gather', 1, 3, 5, 40, 64, '-up', up=1, padx=True),
        _conv('down', 2, 6, 10, 24, 68, entry='down', stride=2, pad_tl=0),
        _conv('fold', 2, 5, 7, 64, 64, '-k64', entry='fold', K2=64),
        # LDS-staged 3x3 conv
        _conv('patch', 3, 8, 8, 64, 68),                                      # ragged N, ragged image groups
        _conv('patch', 5, 4, 4, 128, 132, '-split', rpb=16, res=True, splitk=2, padx=True),
        _conv('patch', 1, 16, 16, 64, 64),                                    # several spatial tiles per image: halos from the neighbouring tile
        _conv('patch', 2, 16, 32, 64, 32),                                    # a tile boundary across the width
    ]


def case_rows(c, rows, supported=None):
    """The rows of the table that case c runs on.  supported(row, c): mkd_gemm_cfg_supported, asked for the LDS-staged rows."""
    if c.kind == 'patch':
        return [r for r in rows if r.family == 'PATCH' and (supported is None or supported(r, c))]
    if c.entry == 'gnstat':
        return [r for r in rows if r.family == 'GEMM']
    if c.kind == 'fold':
        return [r for r in rows if folds_second_input(r)]
    return [r for r in rows if r.family in GATHER_FAMILIES]


def sets_of(c):
    s = ['randn']
    if c.act in (0, 4):
        s.append('exact')
    if c.conv is not None:
        s.append('ones')
    return s


def bit_exact(name, c):
    """exact, and ones without a transcendental activation: every element is compared bit for bit."""
    return name == 'exact' or (name == 'ones' and c.act in (0, 4))


def slabs(c):
    """[[(k0, k1), ...], ...]: the K ranges of every split-K slab in the order the kernels accumulate them (launch_gemm / launch_conv_patch:
    s = min(request, units), per = ceil(units / s), slabs = ceil(units / per); a unit is a 64-wide K-step, on the LDS-staged kernel a
    64-channel chunk with its nine taps)."""
    if c.kind == 'patch':
        units = [[(t * c.conv.Cin + ch * BK, t * c.conv.Cin + ch * BK + BK) for t in range(9)] for ch in range(c.conv.Cin // BK)]
    else:
        units = [[(k, min(k + BK, c.K))] for k in range(0, c.K, BK)]
    assert c.splitk > 0 or len(units) < 8, 'splitk 0 is the heuristic: below 8 K-steps it never splits'
    s = min(max(c.splitk, 1), len(units))
    per = -(-len(units) // s)
    return [sum(units[i:i + per], []) for i in range(0, len(units), per)]


# ---- inputs: dict of fp32 CPU tensors that hold bf16 values -------------------------------------------------------------------------------
EXACT_DENSITY = {}          # case id -> share of non-zero entries of A and W in the exact set (default: all +-1; K <= 1344 here)


def _seed(name, c):
    return 1000 * SETS.index(name) + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % 100000


def build(name, c):
    """x (linear [M, K]; conv [B, H, W, Cin]), w [N, K] (conv: tap-major (ky, kx, ci), then the K2 columns of the second input), x2 [M, K2],
    bias [N], rowbias [samples, N], R [M, N] (None where the case has none) and scale."""
    g = torch.Generator().manual_seed(_seed(name, c))
    cv = c.conv
    xs = (c.M, c.K) if cv is None else (cv.B, cv.H, cv.W, cv.Cin)
    nb = -(-c.M // c.rpb) if c.rpb else 0
    ncol = c.N
    d = dict(x2=None, bias=None, rowbias=None, R=None, scale=c.scale)
    if name == 'randn':
        d['x'] = torch.randn(xs, generator=g)
        d['w'] = torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K)
        if cv is not None and cv.K2:
            d['x2'] = torch.randn(c.M, cv.K2, generator=g)
        small = lambda *s: torch.randn(*s, generator=g)
    else:
        if name == 'exact':
            dens = EXACT_DENSITY.get(c.id, 1.0)
            tern = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).float() * (torch.rand(*s, generator=g) < dens).float()
            d['x'], d['w'] = tern(*xs), tern(c.N, c.K)
            if cv is not None and cv.K2:
                d['x2'] = tern(c.M, cv.K2)
        elif name == 'ones':
            d['x'], d['w'] = torch.ones(xs), torch.full((c.N, c.K), 0.125)
            if cv is not None and cv.K2:
                d['x2'] = torch.ones(c.M, cv.K2)
        else:
            raise ValueError(name)
        small = lambda *s: torch.randint(-3, 4, s, generator=g).float()
        d['scale'] = 1.0 if c.scale == 1.0 else 0.5
    if c.bias:
        d['bias'] = small(ncol)
    if c.rpb:
        d['rowbias'] = small(nb, ncol)
    if c.res:
        d['R'] = small(c.M, ncol)
    for k, v in d.items():
        if torch.is_tensor(v):
            d[k] = q16(v)
    return d


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------
def gather(c, x, x2=None, halo='zero', zero_tap=None):
    """The A matrix [M, K] of the implicit GEMM: row m = output pixel (b, oy, ox), columns (ky, kx, ci) of the 3x3 window whose top-left
    input coordinate, in upsampled space, is (oy stride - pad_tl, ox stride - pad_tl); zeros outside the image; then x2's row.
    Wrong on purpose: halo 'neighbour' reads a row above / below the image from the neighbouring sample (what the flat pixel index
    gives without the range test); zero_tap (m, tap) zeroes one tap of one row."""
    cv = c.conv
    if cv is None:
        return x
    m = torch.arange(c.M)
    hw = cv.Hout * cv.Wout
    b, rem = m // hw, m % hw
    oy, ox = rem // cv.Wout, rem % cv.Wout
    Hup, Wup = cv.H << cv.up, cv.W << cv.up
    flat = x.reshape(cv.B * cv.H * cv.W, cv.Cin)
    cols = []
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        uy, ux = oy * cv.stride - cv.pad_tl + ky, ox * cv.stride - cv.pad_tl + kx
        ok = (uy >= 0) & (uy < Hup) & (ux >= 0) & (ux < Wup)
        sy, sx = torch.div(uy, 1 << cv.up, rounding_mode='floor'), torch.div(ux, 1 << cv.up, rounding_mode='floor')
        idx = (b * cv.H + sy) * cv.W + sx
        if halo == 'neighbour':
            ok = (ux >= 0) & (ux < Wup) & (idx >= 0) & (idx < flat.shape[0])
        v = flat[idx.clamp(0, flat.shape[0] - 1)] * ok[:, None].to(x.dtype)
        if zero_tap is not None and zero_tap[1] == tap:
            v[zero_tap[0]] = 0
        cols.append(v)
    if cv.K2:
        cols.append(x2)
    return torch.cat(cols, 1)


def border_tap(c):
    """(m, tap): the first output pixel with a tap outside the image, and its first tap INSIDE (the zero_tap mutant)."""
    cv = c.conv
    for m in range(c.M):
        rem = m % (cv.Hout * cv.Wout)
        oy, ox = divmod(rem, cv.Wout)
        inside = [0 <= oy * cv.stride - cv.pad_tl + t // 3 < (cv.H << cv.up) and 0 <= ox * cv.stride - cv.pad_tl + t % 3 < (cv.W << cv.up) for t in range(9)]
        if not all(inside):
            return m, inside.index(True)
    raise ValueError('no border pixel')


def _act64(c, z):
    if c.act == 1:
        return z * torch.sigmoid(z)
    if c.act == 3:
        return z * torch.sigmoid(1.702 * z)
    if c.act == 4:
        return z.clamp(min=0)
    if c.act == 2:
        a, g = z[:, 0::2], z[:, 1::2]
        return a * 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))
    return z


def ref(c, d):
    """float64: y [M, N] ([M, N / 2] under GEGLU), the pre-activation z and S [M, N], and the per-element bound of y."""
    A = gather(c, d['x'].double(), None if d['x2'] is None else d['x2'].double())
    W = d['w'].double()
    z, S = A @ W.t(), A.abs() @ W.abs().t()
    if d['bias'] is not None:
        z, S = z + d['bias'].double(), S + d['bias'].double().abs()
    if d['rowbias'] is not None:
        rb = d['rowbias'].double()[torch.arange(c.M) // c.rpb]
        z, S = z + rb, S + rb.abs()
    z, S = z * d['scale'], S * abs(d['scale'])
    if d['R'] is not None:
        z, S = z + d['R'].double(), S + d['R'].double().abs()
    y = _act64(c, z)
    return y, z, S, bound(c, y, z, S)


def bound(c, y, z, S):
    e = (c.K + 4) * U * S
    if c.act in (1, 3):
        k = 1.0 if c.act == 1 else 1.702
        e = LIP_SILU * e + y.abs() * ((k * z).abs() + 3) * U
    elif c.act == 2:
        a, g, ea, eg = z[:, 0::2], z[:, 1::2], e[:, 0::2], e[:, 1::2]
        G = 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))
        dG = 0.5 * g.abs() * ERF_ERR + G.abs() * U
        e = G.abs() * ea + (a.abs() + ea) * (LIP_GELU * eg + dG) + y.abs() * U
    return e + TINY + (0.0 if c.f32 else RND * y.abs())


def ratios(out, y, bnd):
    """|out - y| / bound per element: the bound holds where this is <= 1."""
    return (out.double() - y).abs() / bnd


# ---- where an element lives: tile, wave, fragment ------------------------------------------------------------------------------------------
def patch_geometry(row, c):
    """conv_patch_geometry (kernels_conv.hip): TW = min(W, 16), TH = min(H, TM / TW), IMGS images per block."""
    cv = c.conv
    TW = min(cv.W, 16)
    TH = min(cv.H, row.TM // TW)
    return TH, TW, row.TM // (TH * TW)


def locate(row, c, m, n):
    """'tile (bx, by) wave (wm, wn) fragment (mi, ni)' of output element (m, n) on tile row `row`: block tile TM x TN, WM x WN waves of
    TM / WM x TN / WN each, 16 x 16 fragments.  On the LDS-staged rows a block is a spatial tile of IMGS images and bx its index."""
    if row.family == 'PATCH':
        cv = c.conv
        TH, TW, IM = patch_geometry(row, c)
        b, rem = divmod(m, cv.H * cv.W)
        y, x = divmod(rem, cv.W)
        bx = ((b // IM) * (cv.H // TH) + y // TH) * (cv.W // TW) + x // TW
        lr = (b % IM) * TH * TW + (y % TH) * TW + x % TW
    else:
        bx, lr = divmod(m, row.TM)
    by, lc = divmod(n, row.TN)
    rw, cw = row.TM // row.WM, row.TN // row.WN
    return f'tile ({bx}, {by}) wave ({lr // rw}, {lc // cw}) fragment ({lr % rw // 16}, {lc % cw // 16})'


def report(row, c, name, r):
    """(line, failure or None) for the ratios r [M, N'] of one set: the worst element and where it lives."""
    i = int(r.argmax())
    m, n = divmod(i, r.shape[1])
    ncol = 2 * n if c.act == 2 else n           # (GEGLU: output column n comes from accumulator columns 2n, 2n + 1)
    where = f'element ({m}, {n}) {locate(row, c, m, ncol)}'
    line = f'GEMMEL {row.family} {name} {c.id} row {row.index} {row.name}: worst err / bound {r.max():.3f} at {where}'
    bad = int((~(r <= 1.0)).sum())
    return line, (f'{name}: {bad} elements over the bound, worst {r.max():.2f} at {where}' if bad else None)


# ---- fp32 emulation of the kernels -----------------------------------------------------------------------------------------------------------
def _accumulate(A, W, sl):
    """fp32: every slab accumulates its K-steps in order; the slabs are summed four at a time, then singly (splitk_epilogue_kernel)."""
    parts = []
    for steps in sl:
        acc = torch.zeros(A.shape[0], W.shape[0])
        for k0, k1 in steps:
            acc = acc + A[:, k0:k1] @ W[:, k0:k1].t()
        parts.append(acc)
    v = torch.zeros_like(parts[0]) if len(parts) > 1 else parts[0]
    if len(parts) > 1:
        z = 0
        while z + 4 <= len(parts):
            v = v + ((parts[z] + parts[z + 1]) + (parts[z + 2] + parts[z + 3]))
            z += 4
        for p in parts[z:]:
            v = v + p
    return v


def truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def applies(mutant, c):
    """Whether the fault `mutant` stands for exists in case c."""
    return {'drop_product': True, 'drop_chunk': True, 'zero_tap': c.conv is not None, 'halo_neighbour': c.conv is not None and c.conv.B > 1,
            'truncate': not c.f32, 'residual_after_round': c.res and not c.f32 and c.act == 0, 'rowbias_of_wave': c.rpb > 0 and c.rpb % WAVE_ROWS != 0,
            'skip_bias_tail': c.bias, 'drop_last_slab': len(slabs(c)) > 1}[mutant]


def emulate(c, d, mutant=None):
    """fp32 [M, N] (bf16 values unless c.f32): accumulate in 64-wide K-steps per split-K slab, v + bias, + rowbias, x scale, + R, the
    activation, one rounding.  mutant (wrong on purpose):
      drop_product          one product, k = K / 2, is missing from element (5, 7)
      drop_chunk            the last 16-byte K chunk is not read for the accumulator fragment of rows 16 .. 31, columns 0 .. 15
      zero_tap              one tap inside the image is zero at a border pixel
      halo_neighbour        rows above / below the image come from the neighbouring sample
      truncate              the output is truncated to bf16, not rounded
      residual_after_round  R is added to the rounded value (and the sum rounded again)
      rowbias_of_wave       every 32 rows take the row bias of their first row
      skip_bias_tail        the last 4 columns get no bias
      drop_last_slab        the last split-K slab is never added"""
    assert mutant is None or (mutant in MUTANTS and applies(mutant, c))
    x2 = d['x2']
    A = gather(c, d['x'], x2, halo='neighbour' if mutant == 'halo_neighbour' else 'zero', zero_tap=border_tap(c) if mutant == 'zero_tap' else None)
    W = d['w']
    sl = slabs(c)
    if mutant == 'drop_last_slab':
        sl = sl[:-1]
    v = _accumulate(A, W, sl)
    if mutant == 'drop_product':
        m, n, k = min(5, c.M - 1), min(7, c.N - 1), c.K // 2
        v[m, n] = v[m, n] - A[m, k] * W[n, k]
    if mutant == 'drop_chunk':
        r0, r1 = (16, min(32, c.M)) if c.M > 16 else (0, c.M)
        A2 = A[r0:r1].clone()
        A2[:, c.K - 8:] = 0
        v[r0:r1, :16] = _accumulate(A2, W[:16], sl)
    if d['bias'] is not None:
        b = d['bias'].clone()
        if mutant == 'skip_bias_tail':
            b[-4:] = 0
        v = v + b
    if d['rowbias'] is not None:
        rows = torch.arange(c.M)
        if mutant == 'rowbias_of_wave':
            rows = rows // WAVE_ROWS * WAVE_ROWS
        v = v + d['rowbias'][rows // c.rpb]
    v = v * torch.tensor(d['scale'], dtype=torch.float32)
    if d['R'] is not None and mutant != 'residual_after_round':
        v = v + d['R']
    if c.act == 1:
        v = v * torch.sigmoid(v)
    elif c.act == 3:
        v = v * torch.sigmoid(1.702 * v)
    elif c.act == 4:
        v = v.clamp(min=0)
    elif c.act == 2:
        a, g = v[:, 0::2], v[:, 1::2]
        v = a * (0.5 * g * (1 + torch.erf(g * 0.70710678118654752)))
    if c.f32:
        return v
    if mutant == 'truncate':
        return truncate_bf16(v)
    if mutant == 'residual_after_round':
        return q16(q16(v) + d['R'])
    return q16(v)
