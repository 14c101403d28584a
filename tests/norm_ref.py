"""CPU side of tests/test_gpu_norm_elements.py: the float64 reference of the norm kernels (csrc/kernels_norm.hip)

    GroupNorm   z = (x - mu_g) (var_g + eps)^-1/2 gamma_c + beta_c  [-> SiLU],  statistics over the hw x cg values of (sample, group)
    LayerNorm   the same over the d values of a row

on inputs that are bf16 values already and fp32 affine parameters, plain formulas (no torch norm call); the per-element bound; the
input sets; the shape tables; branch_of / ln_branch_of, a pure-Python mirror of the launchers' arithmetic; an fp32 emulation of a correct
kernel in two summation orders, and emulations that are wrong on purpose (tests/test_norm_ref_host.py shows that the bound separates
them where the suite's global check does not).  No GPU, no library call.

The bound, per element (derived, not measured).  u = 2^-24, K bounds the longest chain of fp32 additions on any path to a group's
sums; from the group's float64 statistics over its n values, S1 = sum |x| / n, S2 = sum x^2 / n, mean mu, variance var:
    one-pass kernels (var = E[x^2] - mean^2 from fp32 sums: every GroupNorm kernel)
        dmu = K u S1                                   the mean
        dv  = K u S2 + 2 |mu| dmu + dmu^2              E[x^2] and the square of the perturbed mean
    two-pass (LayerNorm: the row in registers, centred squares)
        dv  = K u var + dmu^2
    r = (var + eps)^-1/2, r_hi = (max(var - dv, 0) + eps)^-1/2, r_lo = (var + dv + eps)^-1/2     (no first-order step: also right where
                                                       var = 0, a constant or all-zero group, whose reference is exactly beta)
    |dz| <= |gamma| (r_hi dmu + |x - mu| max(r_hi - r, r - r_lo)) + 8 u (|x gamma r| + |mu gamma r| + |beta|)
        the last term: the kernels form x sa + sb with sa = gamma rstd, sb = beta - mean sa - four roundings and rsqrt's, each relative
        to a term that large
    |y - ref| <= L |dz| + 2^-8 |ref| + 2^-20 |z|       L = 1.1 under SiLU (its largest slope, 1.0998), 1 otherwise; one rounding to bf16;
                                                       2^-20 |z|: silu_f's exp2 / rcp (mkd_common.h), relative to its argument
K = 256 for GroupNorm and 64 for LayerNorm are CONDITIONS on the shapes below, not measurements.  Chain lengths read from the kernels:
    gn_fused_kernel, NV = 4 / 8 / 16   <= 16 rows per thread, then 8 channels + a 6-step butterfly + <= 16 waves (register statistics,
                                       cg >= 8: <= 46), or a tree over P <= 341 pixel lanes (9 steps) + cg <= 6 channels (cg < 8: <= 31)
    gn_fused_kernel, NV = 0            ceil(hw / P) rows per thread: 33 at 320 / 1633 (P = 51), 36 at 192 / 3000 (P = 85), then as above (<= 63)
    gn_stats_kernel + gn_apply_kernel  ceil(rows_per_chunk / P) rows per thread (13 at both shapes here) + P cg LDS terms (60 at both)
                                       + 64 chunks: 137
    gn_slab_kernel                     gn_fused_kernel's register statistics, <= 16 rows: <= 46
    gn_colstats_kernel                 ceil(rows_per_block / P) rows per thread (<= 10 here), then 64-bit fixed point: exact sums of
                                       values rounded to 2^-24 (sum) and 2^-18 (squares), at most 2^-19 / rows-per-thread per value of
                                       E[x^2] - below K u S2 = 2^-16 S2 while S2 >= 2^-5 (every group here is above 2^-4)
    layernorm_kernel<NV>               8 NV <= 32 values per lane + a 6-step butterfly: 38
gn_chain(hw, C, groups) computes the GroupNorm figure for a shape; the host test asserts it stays below K on every row.

On the CPU the correct emulation stays within the bound on every row and set (test_norm_ref_host.py re-establishes it); its worst
element is one the bf16 rounding moves by nearly half a unit in the last place (0.99 of the bound)."""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
RND = 2.0 ** -8
ACT = 2.0 ** -20
TINY = 2.0 ** -126
LIP_SILU = 1.1
K_GN = 256
K_LN = 64
GROUPS = 32
SLAB_LIMIT = 384 * 1024
GN_SETS = ('hard', 'offset', 'degenerate', 'far')
LN_SETS = ('hard', 'offset')
GN_MUTANTS = ('drop_last_pixel', 'double_last_pixel', 'stats_of_previous_group', 'stats_of_previous_sample', 'affine_off_by_a_vector',
              'no_silu_on_last_pixel', 'rstd_one')
LN_MUTANTS = ('mean_of_previous_row', 'drop_last_vector')


def q16(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---- the launchers' arithmetic (kernels_norm.hip: gn_block_shape, launch_groupnorm, gn_dispatch_nv, gn_chunk_shape, launch_layernorm) --------
Branch = namedtuple('Branch', 'kernel threads nv stats')          # kernel 'fused' | 'two_kernel'; nv 4 | 8 | 16 | 0 (streaming) | None
Geometry = namedtuple('Geometry', 'kernel threads nv stats gpb V P per nchunks rows_per_chunk')


def gn_block_shape(hw, C, groups, wide=True):
    """(gpb, nt, per) or None: one block per (sample, chunk of gpb groups whose channel span is a multiple of 8)."""
    if groups <= 0 or C % groups:
        return None
    cg = C // groups
    if not wide and cg < 8:
        return None
    gpb = 1
    while gpb <= groups and ((gpb * cg) % 8 or groups % gpb):
        gpb += 1
    if gpb > groups:
        return None
    V = gpb * cg // 8
    if V > 256:
        return None
    per_of = lambda t: -(-hw // (t // V))
    if per_of(256) <= 16:
        return gpb, 256, per_of(256)
    if per_of(512) <= 16:
        return gpb, 512, per_of(512)
    if not wide:
        return None
    if per_of(1024) <= 8:
        return gpb, 1024, per_of(1024)
    return gpb, 256, 1 << 20


def dispatch_nv(per):
    return 4 if per <= 4 else 8 if per <= 8 else 16 if per <= 16 else 0


def gn_chunks(hw):
    return min(max(hw // 16, 1), 64)


def gn_geometry(hw, C, groups=GROUPS):
    """Everything launch_groupnorm decides for a shape."""
    cg = C // groups
    bs = gn_block_shape(hw, C, groups, True)
    if bs is not None and hw * bs[0] * cg * 2 <= SLAB_LIMIT:
        gpb, nt, per = bs
        V = gpb * cg // 8
        return Geometry('fused', nt, dispatch_nv(per), 'register' if cg >= 8 else 'lds_tree', gpb, V, nt // V, per, 0, 0)
    V = C // 8
    P = max(256 // V, 1)
    nch = gn_chunks(hw)
    return Geometry('two_kernel', V * P, None, 'partials', 0, V, P, 0, nch, -(-hw // nch))


def branch_of(hw, C, groups=GROUPS):
    g = gn_geometry(hw, C, groups)
    return Branch(g.kernel, g.threads, g.nv, g.stats)


def slab_branch_of(hw, C):
    """gn_slab_kernel (launch_gn_from_slabs: 32 groups, no 1024-thread or streaming form, cg >= 8) or None."""
    bs = gn_block_shape(hw, C, GROUPS, False)
    return None if bs is None else Branch('slab', bs[1], dispatch_nv(bs[2]), 'register')


def gn_chain(hw, C, groups=GROUPS):
    """The longest chain of fp32 additions from a value to its group's sum."""
    g = gn_geometry(hw, C, groups)
    cg = C // groups
    if g.kernel == 'two_kernel':
        return -(-g.rows_per_chunk // g.P) + g.P * cg + g.nchunks
    rows = g.per if g.nv else -(-hw // g.P)
    if g.stats == 'register':
        return rows + 8 + 6 + g.threads // 64
    return rows + max(g.P - 1, 1).bit_length() + cg


def ln_branch_of(d):
    """(NV, 'full' | 'partial') of layernorm_kernel, or the launcher's error code: one wave per row, lane l holds vectors l + 64 i."""
    if d % 8:
        return -1
    V = d // 8
    if V > 256:
        return -4
    nv = -(-V // 64)
    return nv, 'full' if V == 64 * nv else 'partial'


def _block_lanes(b, r, c, cg, gpb, nt):
    nch = gpb * cg
    P = nt // (nch // 8)
    return f'block ({c // nch}, {b}) vector {(c % nch) // 8} pixel lane {r % P} row slot {r // P}'


def locate(hw, C, b, r, c, groups=GROUPS):
    """Where mkd_groupnorm computes output element (sample b, pixel r, channel c)."""
    g = gn_geometry(hw, C, groups)
    cg = C // groups
    if g.kernel == 'fused':
        where = _block_lanes(b, r, c, cg, g.gpb, g.threads)
    else:
        where = f'block ({r // g.rows_per_chunk}, {b}) vector {c // 8} pixel lane {(r % g.rows_per_chunk) % g.P} row slot {(r % g.rows_per_chunk) // g.P}'
    return f'sample {b} pixel {r} channel {c} group {c // cg}: {where}, branch {tuple(branch_of(hw, C, groups))}'


def locate_slab(hw, C, b, r, c):
    gpb, nt, _ = gn_block_shape(hw, C, GROUPS, False)
    return f'sample {b} pixel {r} channel {c} group {c // (C // GROUPS)}: {_block_lanes(b, r, c, C // GROUPS, gpb, nt)}, branch {tuple(slab_branch_of(hw, C))}'


def locate_stat(case, b, r, c):
    """... in gn_apply_stats_kernel."""
    P, rpb, _ = stat_apply_geometry(case)
    return (f'sample {b} pixel {r} channel {c} group {c // (case.C // GROUPS)}: block ({r // rpb}, {b}) vector {c // 8} pixel lane {(r % rpb) % P} '
            f'row slot {(r % rpb) // P}, branch (apply_stats, {stat_thread_shape(case.C)[0]} threads, {rpb} rows per block)')


def locate_ln(d, row, c):
    return f'row {row} channel {c}: block {row // 4} wave {row % 4} lane {(c // 8) % 64} vector slot {(c // 8) // 64}, branch layernorm_kernel{ln_branch_of(d)}'


def report(tag, r, locate_fn):
    """(line, failure or None) for the ratios r [B, hw, C] (or [rows, d]) of one run: the worst element and where it is computed."""
    i = int(torch.nan_to_num(r, nan=float('inf')).argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    where = locate_fn(*reversed(idx))
    worst = float(torch.nan_to_num(r, nan=float('inf')).max())
    bad = int((~(r <= 1.0)).sum())
    return f'NORMEL {tag}: worst err / bound {worst:.3f} at {where}', (f'{tag}: {bad} elements over the bound, worst {worst:.2f} at {where}' if bad else None)


# ---- the shape tables -------------------------------------------------------------------------------------------------------------------
GnCase = namedtuple('GnCase', 'C hw B silu eps pad sets')
_H, _HOD = ('hard',), ('hard', 'offset', 'degenerate')
GN_CASES = [
    GnCase(320, 16, 2, 1, 1e-5, 0, _H),            # cg 10: 4 groups per block, groups straddle vectors; fused<4>
    GnCase(320, 205, 2, 0, 1e-6, 64, _HOD),        # fused<8>, ragged
    GnCase(320, 409, 2, 1, 1e-5, 0, _H),           # fused<16>, ragged
    GnCase(320, 817, 2, 0, 1e-5, 64, _H),          # fused<16>, 512 threads
    GnCase(320, 1633, 2, 1, 1e-6, 0, _H),          # streaming: the 4-way loop plus a 1-row tail
    GnCase(256, 16, 2, 1, 1e-5, 64, _H),           # cg 8: one vector per group
    GnCase(640, 64, 2, 0, 1e-5, 0, _H),            # cg 20
    GnCase(960, 64, 2, 1, 1e-6, 64, _H),           # cg 30
    GnCase(1920, 64, 2, 1, 1e-5, 0, _H),           # cg 60
    GnCase(2560, 16, 2, 0, 1e-5, 0, _H),           # cg 80: 10 vectors per group
    GnCase(2560, 101, 2, 1, 1e-5, 64, _H),         # fused<8>
    GnCase(64, 64, 2, 1, 1e-5, 0, _H),             # cg 2: the LDS tree, V = 1
    GnCase(128, 64, 2, 0, 1e-6, 64, _H),           # cg 4
    GnCase(192, 100, 2, 1, 1e-5, 0, _HOD),         # cg 6: the LDS tree over P = 85 lanes, not a power of two
    GnCase(192, 2724, 1, 1, 1e-5, 64, _H),         # fused<8>, 1024 threads
    GnCase(192, 3000, 1, 0, 1e-5, 0, _H),          # streaming on the tree
    GnCase(960, 1640, 2, 1, 1e-5, 0, _HOD),        # the two-kernel path, cg >= 8, last chunk of 2 rows
    GnCase(192, 8200, 1, 1, 1e-6, 0, _H),          # the two-kernel path, cg < 8
]
FAR_GN = [(320, 205), (960, 1640)]                 # rows that also run the far set (measured)
GN_BRANCHES = {Branch('fused', 256, 4, 'register'), Branch('fused', 256, 8, 'register'), Branch('fused', 256, 16, 'register'),
               Branch('fused', 256, 0, 'register'), Branch('fused', 512, 16, 'register'), Branch('fused', 1024, 8, 'lds_tree'),
               Branch('fused', 256, 4, 'lds_tree'), Branch('fused', 256, 0, 'lds_tree'),
               Branch('two_kernel', 240, None, 'partials')}


def gn_id(c):
    return f'C{c.C}-hw{c.hw}-B{c.B}'


# mkd_gn_colstats (two column slices [0, split), [split, C)) + mkd_gn_apply_stats
StatCase = namedtuple('StatCase', 'C hw B split silu eps pad sets')
STAT_CASES = [
    StatCase(64, 600, 2, 16, 1, 1e-5, 0, ('hard', 'exact')),                         # slices of 2 and 6 vectors: 2 and 4 ragged blocks per sample
    StatCase(320, 100, 2, 104, 1, 1e-5, 64, ('hard', 'degenerate', 'far', 'exact')),      # several blocks per sample in both kernels, a ragged last one
    StatCase(1280, 1100, 2, 424, 0, 1e-6, 0, ('hard',)),                             # apply: 5 rows per block at P = 1, the prefetch loop runs twice
    StatCase(2560, 37, 2, 848, 1, 1e-5, 64, ('hard', 'exact')),                      # 320 threads, one pixel lane
]


def stat_thread_shape(cols):
    """gn_thread_shape: (threads, P)."""
    V = cols // 8
    P = 1 if V >= 256 else 256 // V
    return V * P, P


def stat_apply_geometry(c):
    """launch_gn_apply_stats: (P, rows per block, blocks per sample)."""
    _, P = stat_thread_shape(c.C)
    rpb = max(-(-(-(-c.B * c.hw // 512)) // P) * P, P)
    return P, rpb, -(-c.hw // rpb)


def stat_colstats_geometry(c, ncols):
    _, P = stat_thread_shape(ncols)
    rpb = max(-(-(-(-c.B * c.hw // 256)) // P) * P, 4 * P)
    return P, rpb, -(-c.hw // rpb)


# mkd_gemm_groupnorm_bf16: a 3x3 conv, Cin 64 -> Cout 320, split over K in 2, B = 2
SlabCase = namedtuple('SlabCase', 'H W silu eps')
SLAB_CASES = [SlabCase(8, 8, 1, 1e-5), SlabCase(16, 16, 0, 1e-6), SlabCase(32, 32, 1, 1e-5)]
SLAB_CIN, SLAB_COUT, SLAB_B, SLAB_SPLITK = 64, 320, 2, 2

LN_ROWS = (5, 37)
LN_D = (64, 320, 512, 640, 1024, 1280, 1536, 1600, 2048)          # (1536: the only full last vector of layernorm_kernel<3>)
LN_BRANCHES = {(nv, f) for nv in (1, 2, 3, 4) for f in ('full', 'partial')}
LN_ERRORS = {2056: -4, 324: -1}


# ---- inputs: fp32 CPU tensors that hold bf16 values ---------------------------------------------------------------------------------------
def _seed(*key):
    s = '/'.join(str(k) for k in key)
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(s)) % 1000003


def affine(n, seed):
    g = torch.Generator().manual_seed(_seed('affine', n, seed))
    return 1 + 0.2 * torch.randn(n, generator=g), 0.2 * torch.randn(n, generator=g)


def _levels(name, g, count):
    """(std, mean / std) per statistics unit: std = 2^k with every k of -2 .. 2 in turn; mean / std uniform in +-4 (hard, degenerate),
    +-16 with both ends present (offset), +-100 exactly (far)."""
    k = (torch.arange(count) * 3 % 5 - 2).double()
    m = torch.rand(count, generator=g, dtype=torch.float64) * 2 - 1
    if name in ('hard', 'degenerate'):
        m = m * 4
    elif name == 'offset':
        m = m * 16
        m[0], m[1] = 16.0, -16.0
    elif name == 'far':
        m = torch.where(torch.arange(count) % 2 == 0, 100.0, -100.0).double()
    else:
        raise ValueError(name)
    return 2.0 ** k, m


def degenerate_groups(b):
    """(all-zero group, group constant at 3.0, group constant at -100) of sample b."""
    return (3 + 5 * b) % GROUPS, (11 + 7 * b) % GROUPS, (20 + 3 * b) % GROUPS


def gn_input(name, B, hw, C, groups=GROUPS):
    """x [B, hw, C]: every (sample, group) with its own mean and scale, pixel 0 of every sample shifted by +6 standard deviations and the
    last pixel by -6 (a pixel that is dropped, doubled or given to the wrong chunk moves the statistics by many bounds)."""
    g = torch.Generator().manual_seed(_seed('gn', name, B, hw, C))
    cg = C // groups
    if name == 'iid':          # the existing tests' inputs
        return q16(torch.randn(B, hw, C, generator=g) * 2 + 0.5)
    if name == 'exact':        # small integers: every sum is exact
        return torch.randint(-8, 9, (B, hw, C), generator=g).float()
    std, m = _levels(name, g, B * groups)
    std, m = std.view(B, 1, groups, 1), m.view(B, 1, groups, 1)
    x = torch.randn(B, hw, groups, cg, generator=g, dtype=torch.float64)
    x[:, 0] += 6
    x[:, -1] -= 6
    x = (x + m) * std
    if name == 'degenerate':
        for b in range(B):
            z, c3, c100 = degenerate_groups(b)
            x[b, :, z], x[b, :, c3], x[b, :, c100] = 0.0, 3.0, -100.0
    return q16(x.reshape(B, hw, C).float())


def ln_input(name, rows, d):
    """x [rows, d]: every row with its own mean and scale (hard: mean within 4 standard deviations; offset: row means up to +-50, the
    kernel is two-pass), the first and last 8 channels of every row shifted by +-6 standard deviations."""
    g = torch.Generator().manual_seed(_seed('ln', name, rows, d))
    if name == 'iid':
        return q16(torch.randn(rows, d, generator=g) * 3 + 1)
    std, m = _levels('hard', g, rows)
    x = torch.randn(rows, d, generator=g, dtype=torch.float64)
    x[:, :8] += 6
    x[:, -8:] -= 6
    if name == 'offset':
        mean = torch.rand(rows, generator=g, dtype=torch.float64) * 100 - 50
        mean[0], mean[1] = 50.0, -50.0
        x = x * std[:, None] + mean[:, None]
    else:
        x = (x + m[:, None]) * std[:, None]
    return q16(x.float())


def slab_operands(c):
    """The operands of a 3x3 conv (an implicit GEMM over K = 9 Cin) whose OUTPUT has hard per-(sample, group) statistics: the weights of
    output group g scaled by 2^k, k in -2 .. 2 in turn; a bias per group within 4 of those standard deviations; a row bias per sample,
    +-3 of them.  x [B, H, W, Cin], w [Cout, 9 Cin] (bf16 values), bias [Cout], rowbias [B, Cout] (fp32)."""
    g = torch.Generator().manual_seed(_seed('slab', c.H, c.W))
    K, cg = 9 * SLAB_CIN, SLAB_COUT // GROUPS
    std, m = _levels('hard', g, GROUPS)
    std, m = std.float().repeat_interleave(cg), m.float().repeat_interleave(cg)
    x = q16(torch.randn(SLAB_B, c.H, c.W, SLAB_CIN, generator=g))
    w = q16(torch.randn(SLAB_COUT, K, generator=g) / math.sqrt(K) * std[:, None])
    shift = torch.tensor([3.0, -3.0])[:SLAB_B]
    return x, w, m * std, shift[:, None] * std[None, :]


# ---- the float64 reference and the bound ---------------------------------------------------------------------------------------------------
def _bound(x, mu, var, S1, S2, gamma, beta, eps, silu, K, one_pass):
    dmu = K * U * S1
    dv = K * U * S2 + 2 * mu.abs() * dmu + dmu ** 2 if one_pass else K * U * var + dmu ** 2
    r = (var + eps) ** -0.5
    r_hi = ((var - dv).clamp(min=0) + eps) ** -0.5
    r_lo = (var + dv + eps) ** -0.5
    z = (x - mu) * r * gamma + beta
    dz = gamma.abs() * (r_hi * dmu + (x - mu).abs() * torch.maximum(r_hi - r, r - r_lo)) + \
        8 * U * ((x * gamma * r).abs() + (mu * gamma * r).abs() + beta.abs())
    ref = z * torch.sigmoid(z) if silu else z
    return ref, (LIP_SILU if silu else 1.0) * dz + RND * ref.abs() + ACT * z.abs() + TINY


def gn_ref(x, gamma, beta, eps, silu, groups=GROUPS, K=K_GN):
    """float64 (ref, bound) [B, hw, C] of GroupNorm [+SiLU] over x [B, hw, C] (bf16 values)."""
    B, hw, C = x.shape
    xg = x.double().view(B, hw, groups, C // groups)
    mu = xg.mean((1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean((1, 3), keepdim=True)
    S1, S2 = xg.abs().mean((1, 3), keepdim=True), (xg ** 2).mean((1, 3), keepdim=True)
    ga, be = gamma.double().view(1, 1, groups, -1), beta.double().view(1, 1, groups, -1)
    ref, bnd = _bound(xg, mu, var, S1, S2, ga, be, eps, silu, K, True)
    return ref.reshape(B, hw, C), bnd.reshape(B, hw, C)


def ln_ref(x, gamma, beta, eps, K=K_LN):
    """float64 (ref, bound) [rows, d] of LayerNorm over x [rows, d]."""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    return _bound(xd, mu, var, xd.abs().mean(1, keepdim=True), (xd ** 2).mean(1, keepdim=True), gamma.double(), beta.double(), eps, 0, K, False)


def ratios(out, ref, bnd):
    """|out - ref| / bound per element: the bound holds where this is <= 1 (a NaN counts as over)."""
    return (out.double() - ref).abs() / bnd


def group_rel_l2(out, ref, groups=GROUPS):
    """rel-L2 per (sample, group) of [B, hw, C] tensors."""
    B, hw, C = ref.shape
    e = (out.double() - ref).view(B, hw, groups, -1)
    return (e.pow(2).sum((1, 3)) / ref.view(B, hw, groups, -1).pow(2).sum((1, 3)).clamp(min=1e-300)).sqrt()


# ---- fp32 emulation of the kernels -----------------------------------------------------------------------------------------------------------
def _sums(x, groups, order):
    """fp32 (sum, sum of squares) [B, groups] of x [B, hw, C] (fp32).  'chunked': 64 pixel lanes take every 64th row one after the other, a
    pairwise sum over the lanes, then over the group's channels (the shape of the kernels' sums).  'sequential': one chain over the
    pixels of a channel, then one over the group's channels.  'any': torch's own order (the emulations that are wrong on purpose)."""
    B, hw, C = x.shape
    if order == 'any':
        xg = x.view(B, hw, groups, -1)
        return xg.sum((1, 3)), (xg * xg).sum((1, 3))
    if order == 'sequential':
        s, q = torch.zeros(B, C), torch.zeros(B, C)
        for r in range(hw):
            s = s + x[:, r]
            q = q + x[:, r] * x[:, r]
        sg, qg = s.view(B, groups, -1), q.view(B, groups, -1)
        a, b = torch.zeros(B, groups), torch.zeros(B, groups)
        for j in range(sg.shape[2]):
            a = a + sg[:, :, j]
            b = b + qg[:, :, j]
        return a, b
    P = 64
    rows = -(-hw // P)
    xp = torch.zeros(B, rows * P, C)
    xp[:, :hw] = x
    xp = xp.view(B, rows, P, C)
    s, q = torch.zeros(B, P, C), torch.zeros(B, P, C)
    for i in range(rows):
        s = s + xp[:, i]
        q = q + xp[:, i] * xp[:, i]
    return s.sum(1).view(B, groups, -1).sum(2), q.sum(1).view(B, groups, -1).sum(2)


def gn_applies(mutant, B, silu):
    return {'stats_of_previous_sample': B > 1, 'no_silu_on_last_pixel': bool(silu)}.get(mutant, True)


def gn_emulate(x, gamma, beta, eps, silu, groups=GROUPS, order='chunked', mutant=None):
    """fp32 emulation of a one-pass GroupNorm kernel: fp32 sums, mean = s / n, var = max(q / n - mean^2, 0), rstd = (var + eps)^-1/2,
    y = bf16(act(x sa + sb)) with sa = gamma rstd, sb = beta - mean sa.  mutant (wrong on purpose):
      drop_last_pixel            the last pixel of every sample is left out of the statistics
      double_last_pixel          ... counted twice
      stats_of_previous_group    group g normalises with the statistics of group g - 1
      stats_of_previous_sample   sample b with those of sample b - 1
      affine_off_by_a_vector     channel c takes gamma / beta of channel c - 8
      no_silu_on_last_pixel      SiLU skipped on the last pixel
      rstd_one                   rstd = 1 although the group's sum of squares is not zero (the q == 0 branch of gn_apply_stats_kernel taken
                                 wrongly)"""
    assert mutant is None or (mutant in GN_MUTANTS and gn_applies(mutant, x.shape[0], silu))
    B, hw, C = x.shape
    cg = C // groups
    x = x.float()
    xs = x
    if mutant == 'drop_last_pixel':
        xs = x[:, :-1]
    elif mutant == 'double_last_pixel':
        xs = torch.cat([x, x[:, -1:]], 1)
    s, q = _sums(xs.contiguous(), groups, order if mutant is None else 'any')
    n = torch.tensor(float(hw) * float(cg), dtype=torch.float32)
    mean = s / n
    var = (q / n - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    if mutant == 'rstd_one':
        rstd = torch.where(q != 0, torch.ones_like(rstd), rstd)
    if mutant == 'stats_of_previous_group':
        mean, rstd = mean.roll(1, 1), rstd.roll(1, 1)
    if mutant == 'stats_of_previous_sample':
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    ga, be = gamma.float(), beta.float()
    if mutant == 'affine_off_by_a_vector':
        ga, be = ga.roll(8), be.roll(8)
    sa = ga.view(1, groups, cg) * rstd.view(B, groups, 1)
    sb = be.view(1, groups, cg) - mean.view(B, groups, 1) * sa
    f = x.view(B, hw, groups, cg) * sa.view(B, 1, groups, cg) + sb.view(B, 1, groups, cg)
    if silu:
        a = f * torch.sigmoid(f)
        if mutant == 'no_silu_on_last_pixel':
            a[:, -1] = f[:, -1]
        f = a
    return q16(f.reshape(B, hw, C))


def ln_emulate(x, gamma, beta, eps, order='chunked', mutant=None):
    """fp32 emulation of layernorm_kernel: mean, then the centred squares, y = bf16((x - mean) rstd gamma + beta).  'chunked': 64 lanes
    take every 64th vector, pairwise over the lanes; 'sequential': one chain along the row.  mutant:
      mean_of_previous_row   row r is centred on the mean of row r - 1
      drop_last_vector       the last 8 channels are left out of both sums"""
    assert mutant is None or mutant in LN_MUTANTS
    rows, d = x.shape
    x = x.float()
    keep = d - 8 if mutant == 'drop_last_vector' else d

    def total(t):
        t = t[:, :keep]
        if order == 'sequential':
            return t.cumsum(1)[:, -1] if mutant is None else t.sum(1)
        w = -(-t.shape[1] // 512) * 512
        tp = torch.zeros(rows, w)
        tp[:, :t.shape[1]] = t
        tp = tp.view(rows, w // 512, 64, 8)
        acc = torch.zeros(rows, 64)
        for i in range(w // 512):
            for j in range(8):
                acc = acc + tp[:, i, :, j]
        return acc.sum(1)

    dn = torch.tensor(float(d), dtype=torch.float32)
    mean = (total(x) / dn)[:, None]
    if mutant == 'mean_of_previous_row':
        mean = mean.roll(1, 0)
    c = x - mean
    rstd = 1.0 / torch.sqrt(total(c * c) / dn + torch.tensor(eps, dtype=torch.float32))
    return q16(c * rstd[:, None] * gamma.float() + beta.float())
