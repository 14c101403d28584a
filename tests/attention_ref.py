"""CPU side of tests/test_gpu_attention.py: the float64 reference of softmax(Q K^T scale) V per (sample, head), the input sets that
make one fault of the kernels in csrc/kernels_attn.hip the whole error of some row, the per-row bound, the list of cases (one per
dispatch branch of launch_attention and boundary) and tile-wise emulations of the online softmax - a correct one and six that are
wrong on purpose (tests/test_attention_ref_host.py shows that the bound separates them).  No GPU, no library call.

The bound, per (query row, head):      max_d |out - ref| <= 2^-7 A,      A = max_d sum_j p_j |v_jd|   ("absolute-value attention")
    2 x 2^-9 A   P is rounded to bf16 in the numerator and, at worst, not in the denominator
        2^-9 A   the output is rounded to bf16
        2^-9 A   fp32 score accumulation and v_exp_f32, for |score scale log2(e)| <= 256 (SCORE_CAP: every builder keeps it)
It is derived, not measured: the correct emulation below reaches at most 0.61 of 3 x 2^-9 A on every set (0.75 with the lazy bf16
reference of the dh-40 long path, whose weights reach 2^6 before the rescale), i.e. 0.56 of the bound."""
import itertools
import math
from collections import namedtuple

import torch

LOG2E = 1.4426950408889634
BOUND = 2.0 ** -7
SCORE_CAP = 256.0
SETS = ('soft', 'hard', 'uniform', 'ascending', 'descending', 'padding_would_win', 'designated')
MUTANTS = ('droplast', 'droptile', 'norescale', 'swapheads', 'nocausal', 'clamp')


def q16(t):
    return t.to(torch.bfloat16).float()


def _split(x, B, T, heads, dh):
    return x.reshape(B, T, heads, dh).permute(0, 2, 1, 3)           # [B, heads, T, dh]


def _merge(x):
    B, H, T, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * dh)


def scale_log2e_f32(scale):
    """The factor as the launcher forms it: float(scale) * 1.4426950408889634f, in fp32."""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def prescaled_queries(q, scale):
    """AttnCfg::OFFS (the dh-40 long path): q' = bf16(float32(q) * scale_log2e); the scores are q'.k, already in the log2 domain."""
    return q16(q.float() * scale_log2e_f32(scale))


def visible(Tq, Tk, causal):
    """[Tq, Tk] bool.  Causal, as the kernel has it: query i sees keys 0 .. min(i, Tk - 1)."""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    lim = torch.arange(Tq).clamp(max=Tk - 1)
    return torch.arange(Tk)[None, :] <= lim[:, None]


def scores_log2(q, k, B, Tq, Tk, heads, dh, scale, prescale=False):
    """[B, heads, Tq, Tk] float64: score * scale * log2(e) on inputs that are bf16 values already."""
    kh = _split(k.double(), B, Tk, heads, dh)
    if prescale:
        return _split(prescaled_queries(q, scale).double(), B, Tq, heads, dh) @ kh.transpose(-1, -2)
    return (_split(q.double(), B, Tq, heads, dh) @ kh.transpose(-1, -2)) * float(scale_log2e_f32(scale).double())


def weights(q, k, B, Tq, Tk, heads, dh, scale, causal=False, prescale=False):
    s = scores_log2(q, k, B, Tq, Tk, heads, dh, scale, prescale).masked_fill(~visible(Tq, Tk, causal), -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True), s


def ref(q, k, v, B, Tq, Tk, heads, dh, scale, causal=False, prescale=False):
    """float64 on the bf16-rounded inputs: out [B*Tq, d] and A [B*Tq, heads].  prescale: the emulated-query reference of the dh-40
    long path (the kernel's documented input rounding); without it the exact one."""
    p, _ = weights(q, k, B, Tq, Tk, heads, dh, scale, causal, prescale)
    vh = _split(v.double(), B, Tk, heads, dh)
    out = _merge(p @ vh)
    A = (p @ vh.abs()).amax(-1).permute(0, 2, 1).reshape(B * Tq, heads)
    return out, A


def row_err(out, want, heads, dh):
    """[rows, heads]: max over the head's channels of |out - ref|."""
    return (out.double() - want.double()).abs().reshape(-1, heads, dh).amax(-1)


def ratios(out, want, A, heads, dh):
    """err / (2^-7 A) per (row, head): the bound holds where this is <= 1."""
    return row_err(out, want, heads, dh) / (BOUND * A)


# ---- the cases: one per dispatch branch and boundary (the conditions are launch_attention's) --------------------------------------
Case = namedtuple('Case', 'branch B Tq Tk heads dh causal tile separate')
DHS = (8, 16, 32, 40, 64, 80, 160)
TILE = {'G': 64, 'C': 96, 'W0': 64, 'W1': 64, 'D': 128, 'K': 64}


def branch_of(Tq, Tk, dh, causal):
    """The path launch_attention takes in the default build, and its key tile."""
    wide = Tq >= 1024 and Tk >= 1024
    if causal:
        return 'K'
    if wide:
        return 'D' if dh == 40 else ('W1' if Tk >= 2048 else 'W0')
    return 'C' if 64 < Tk <= 96 else 'G'


def cases():
    out = []
    G_TK = (1, 15, 16, 17, 31, 32, 33, 63, 64, 97, 127, 128, 129, 200)
    for dh in (40, 160):
        out += [('G', 2, Tq, Tk, 2, dh, 0) for Tk in G_TK for Tq in (1, 63, 64, 65, 100)]
    out += [('G', 2, 100, Tk, 2, dh, 0) for dh in (8, 16, 32, 64, 80) for Tk in (17, 64, 129)]
    out += [('C', 2, Tq, Tk, 2, dh, 0) for dh in DHS for Tk in (65, 77, 79, 80, 81, 95, 96) for Tq in (16, 100)]
    out += [('W0', 1, 1040, 1025, 2, dh, 0) for dh in (8, 16, 32, 64, 80, 160)]
    out += [('W0', 1, 1040, Tk, 2, 80, 0) for Tk in (1087, 1088)]
    out += [('W1', 1, 1040, 2049, 1, dh, 0) for dh in (8, 16, 32, 64, 80, 160)]
    out += [('D', 1, Tq, Tk, 2, 40, 0) for Tq in (1024, 1040) for Tk in (1024, 1025, 1151, 1152, 1153)]
    out += [('D', 2, 1040, 1153, 2, 40, 0)]
    out += [('K', 2, Tq, Tk, 2, dh, 1) for dh in (64, 40) for Tq, Tk in ((77, 77), (100, 64), (64, 100), (1, 1), (130, 130))]
    out += [('K', 1, 1040, 1040, 1, 64, 1)]
    seen, res = set(), []
    for br, B, Tq, Tk, heads, dh, causal in out:
        res.append(Case(br, B, Tq, Tk, heads, dh, causal, TILE[br], br not in seen))      # the first of a branch: K and V as separate tensors
        seen.add(br)
    return res


def case_id(c):
    return f'{c.branch}-B{c.B}-Tq{c.Tq}-Tk{c.Tk}-h{c.heads}-dh{c.dh}'


def sets_of(c):
    s = ['soft', 'hard', 'uniform', 'padding_would_win']
    if c.Tk > c.tile:
        s += ['ascending', 'descending']
    if c.dh >= 32 or c.branch not in ('W0', 'W1'):
        s.append('designated')
    return s


# ---- input builders: seeded, fp32 [B*Tq, d], [B*Tk, d], [B*Tk, d] and the scale; the tests round them to bf16 -----------------------
def make_v(B, Tk, heads, dh, g):
    """randn; channel 0 of every head = the key ramp j / Tk; channel 1 = the code b * heads + h + 1 (a head or sample mix-up shows in
    this channel alone)."""
    v = torch.randn(B, Tk, heads, dh, generator=g)
    v[..., 0] = (torch.arange(Tk, dtype=torch.float32) / Tk)[None, :, None]
    v[..., 1] = (torch.arange(B)[:, None] * heads + torch.arange(heads)[None, :] + 1).float()[:, None, :]
    return v.reshape(B * Tk, heads * dh)


def lattice(n, count):
    """count points of {-1, 0, 1}^n, by rising norm: the origin, +-e_i, +-e_i +-e_j, ...  Any two differ by at least 1."""
    pts = []
    for r in range(n + 1):
        for idx in itertools.combinations(range(n), r):
            for sg in itertools.product((-1.0, 1.0), repeat=r):
                p = [0.0] * n
                for i, s in zip(idx, sg):
                    p[i] = s
                pts.append(p)
                if len(pts) == count:
                    return torch.tensor(pts)
    raise ValueError(f'{count} points do not fit {{-1, 0, 1}}^{n}')


def must_cover(Tk, tile):
    """Keys a designated set has to reach when there are fewer queries than keys, first things first: the last key, key 0, then every
    multiple of 16, 32 and the tile below Tk with both of its neighbours."""
    keys = [Tk - 1, 0]
    for m in sorted({m for step in (16, 32, tile) for m in range(step, Tk, step)}, reverse=True):
        keys += [m - 1, m + 1, m]
    out = []
    for j in keys:
        if 0 <= j < Tk and j not in out:
            out.append(j)
    return out


DESIGNATED_SCALE = 24.0


def designated_keys(B, Tq, Tk, heads, tile, causal, seed):
    """[B, heads, Tq]: the key every query puts its weight on.  Tq >= Tk: every key is some query's, in every (sample, head).  Causal:
    query i < Tk takes key i, the last one it sees.  Tq < Tk: the must_cover list, rotated per (sample, head), then seeded draws; with
    fewer queries than the list is long (Tq = 1) its head, so that the (sample, head)s between them still reach the last key and key 0."""
    g = torch.Generator().manual_seed(seed + 1)
    key = torch.empty(B, heads, Tq, dtype=torch.long)
    must = must_cover(Tk, tile)
    for b in range(B):
        for h in range(heads):
            off = b * heads + h
            i = torch.arange(Tq)
            if causal:
                rest = torch.minimum(torch.randint(0, Tk, (Tq,), generator=g), i)
                key[b, h] = torch.where(i < Tk, i, rest)
            elif Tq >= Tk:
                key[b, h] = (i + 7 * off) % Tk
            else:
                kk = torch.randint(0, Tk, (Tq,), generator=g)
                n = min(Tq, len(must))
                kk[:n] = torch.tensor([must[(j + off) % len(must)] for j in range(n)])
                key[b, h] = kk
    return key


def designated(B, Tq, Tk, heads, dh, tile, causal, seed):
    """k_j = (u_j, -|u_j|^2 / 2) with u_j lattice points (shuffled per (sample, head)), q_i = (u_key(i), 1): score = -|u_key(i) - u_j|^2 / 2
    + const, so the designated key leads every other by scale / 2 = 12 in natural units.  All values are bf16-exact; the scale is the
    ABI's argument."""
    g = torch.Generator().manual_seed(seed)
    pts = lattice(dh - 1, Tk)
    key = designated_keys(B, Tq, Tk, heads, tile, causal, seed)
    q = torch.empty(B, Tq, heads, dh)
    k = torch.empty(B, Tk, heads, dh)
    for b in range(B):
        for h in range(heads):
            u = pts[torch.randperm(Tk, generator=g)]
            k[b, :, h, :dh - 1] = u
            k[b, :, h, dh - 1] = -0.5 * (u * u).sum(-1)
            q[b, :, h, :dh - 1] = u[key[b, h]]
            q[b, :, h, dh - 1] = 1.0
    d = heads * dh
    return q.reshape(B * Tq, d), k.reshape(B * Tk, d), make_v(B, Tk, heads, dh, g), DESIGNATED_SCALE


def tile_levels(Tk, tile):
    """log2-domain level of every key: constant inside a key tile, rising by 3 and 9 in turn from tile to tile (below and above the
    lazy reference's threshold of 6: the dh-40 path sees both of its branches), centred so that the score cap holds."""
    nt = (Tk + tile - 1) // tile
    lev = torch.tensor([0.0] + [3.0 if t % 2 else 9.0 for t in range(1, nt)]).cumsum(0)
    lev = lev - 0.5 * lev[-1]
    return lev[torch.arange(Tk) // tile]


def ramped(B, Tq, Tk, heads, dh, tile, seed, descending):
    """A shared direction e (signs): q = e + 0.1 randn, k_j = level_j e / (dh scale log2 e) + 0.25 randn.  Ascending: the row maximum
    moves to a later key in every tile, the rescale runs every tile; descending: never after tile 0."""
    g = torch.Generator().manual_seed(seed)
    scale = dh ** -0.5
    e = torch.randint(0, 2, (heads, dh), generator=g).float() * 2 - 1
    lev = tile_levels(Tk, tile)
    if descending:
        lev = -lev
    q = e[None, None] + 0.1 * torch.randn(B, Tq, heads, dh, generator=g)
    k = (lev / (dh * scale * LOG2E))[None, :, None, None] * e[None, None] + 0.25 * torch.randn(B, Tk, heads, dh, generator=g)
    d = heads * dh
    return q.reshape(B * Tq, d), k.reshape(B * Tk, d), make_v(B, Tk, heads, dh, g), scale


def build_seed(name, c, seed=0):
    return seed + 1000 * SETS.index(name) + 7 * c.Tq + 13 * c.Tk + c.dh


def build(name, c, seed=0):
    """(q, k, v, scale) of set `name` for case c."""
    B, Tq, Tk, heads, dh = c.B, c.Tq, c.Tk, c.heads, c.dh
    d = heads * dh
    seed = build_seed(name, c, seed)
    g = torch.Generator().manual_seed(seed)
    if name == 'designated':
        return designated(B, Tq, Tk, heads, dh, c.tile, c.causal, seed)
    if name in ('ascending', 'descending'):
        return ramped(B, Tq, Tk, heads, dh, c.tile, seed, name == 'descending')
    if name in ('soft', 'hard'):
        q = torch.randn(B * Tq, d, generator=g) * (4.0 if name == 'hard' else 1.0)
        return q, torch.randn(B * Tk, d, generator=g), make_v(B, Tk, heads, dh, g), dh ** -0.5
    if name == 'uniform':                       # q = 0: the output is the mean of V over the visible keys
        return torch.zeros(B * Tq, d), torch.randn(B * Tk, d, generator=g), make_v(B, Tk, heads, dh, g), dh ** -0.5
    if name == 'padding_would_win':             # every real score ~ -20 (natural units); a zero-padded key would score 0 and take the row
        q = 1.0 + 0.05 * torch.randn(B * Tq, d, generator=g)
        k = -3.0 + 0.1 * torch.randn(B * Tk, d, generator=g)
        return q, k, make_v(B, Tk, heads, dh, g), 20.0 / (3.0 * dh)
    raise ValueError(name)


# ---- tile-wise emulations of the kernels' online softmax ----------------------------------------------------------------------------
def emulate(q, k, v, c, scale, mode='plain', mutant=None, mtile=1):
    """fp32 online softmax over key tiles of c.tile with P rounded to bf16 for P.V and a bf16 output, [B*Tq, d].
    mode  plain  running maximum, denominator from the unrounded p (attention_kernel)
          msum   ... denominator from the rounded p (AttnCfg::ONES)
          dma    pre-scaled bf16 queries, a lazily updated bf16 reference in place of the maximum, denominator from the rounded p
    mutant (wrong on purpose)  droplast: the last key is never read;  droptile: key tile mtile is skipped;  norescale: the rescale of
    O and of the denominator is skipped in tile mtile;  swapheads: V of the next head;  nocausal: the causal limit ignored;  clamp: a
    partial last tile is filled with copies of the last valid key and not masked."""
    assert mutant is None or mutant in MUTANTS
    B, Tq, Tk, heads, dh, tile = c.B, c.Tq, c.Tk, c.heads, c.dh, c.tile
    sl = scale_log2e_f32(scale)
    qh = _split(q16(q), B, Tq, heads, dh)
    kh = _split(q16(k), B, Tk, heads, dh)
    vh = _split(q16(v), B, Tk, heads, dh)
    if mutant == 'swapheads':
        vh = vh.roll(1, dims=1)
    if mutant == 'droplast':
        kh, vh, Tk = kh[:, :, :Tk - 1], vh[:, :, :Tk - 1], Tk - 1
    if mode == 'dma':
        qh = q16(qh * sl)
    vis = visible(Tq, Tk, c.causal and mutant != 'nocausal')
    shape = (B, heads, Tq)
    m = torch.full(shape, -math.inf)
    mref = torch.zeros(shape)
    l = torch.zeros(shape)
    o = torch.zeros(B, heads, Tq, dh)
    first = True
    ntiles = (Tk + tile - 1) // tile
    mtile = mtile % ntiles                        # (-1: the last tile)
    for t in range(ntiles):
        if mutant == 'droptile' and t == mtile:
            continue
        k0, k1 = t * tile, min((t + 1) * tile, Tk)
        kt, vt, vs = kh[:, :, k0:k1], vh[:, :, k0:k1], vis[:, k0:k1]
        if mutant == 'clamp' and k1 - k0 < tile:
            n = tile - (k1 - k0)
            kt = torch.cat([kt, kt[:, :, -1:].expand(-1, -1, n, -1)], 2)
            vt = torch.cat([vt, vt[:, :, -1:].expand(-1, -1, n, -1)], 2)
            vs = torch.cat([vs, vs[:, -1:].expand(-1, n)], 1)
        s = (qh @ kt.transpose(-1, -2)).masked_fill(~vs, -math.inf)
        if mode == 'dma':
            s = s - mref[..., None]
            mx = s.amax(-1)
            need = (mx > 6.0) | first
            m_new = torch.where(need, q16(mref + mx), mref)
            alpha = torch.exp2(mref - m_new)
            p = torch.exp2(s - (m_new - mref)[..., None])
            mref = m_new
        else:
            m_new = torch.maximum(m, s.amax(-1) * sl)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(s * sl - m_new[..., None])
            m = m_new
        first = False
        pb = q16(p)
        if not (mutant == 'norescale' and t == mtile):
            o = o * alpha[..., None]
            l = l * alpha
        o = o + pb @ vt
        l = l + (p if mode == 'plain' else pb).sum(-1)
    return q16(_merge(o / l[..., None]))
