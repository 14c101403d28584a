"""No GPU: the shape tables, input sets and bound of tests/norm_ref.py do what tests/test_gpu_norm_elements.py relies on.  The shape tables
reach every branch of the launchers (asserted through branch_of / ln_branch_of, the Python mirror of their arithmetic) and keep every
chain of fp32 additions below the K of the bound; the float64 reference agrees with torch's group_norm / layer_norm; an fp32 emulation of a
correct kernel stays within the per-element bound on every row and set, in two summation orders; every emulation that is wrong on
purpose is flagged by the bound on EVERY row where the fault exists.  test_every_mutant_is_flagged_on_every_row also prints, per mutant,
on how many rows the suite's global check (assert_close_bf16: rel-L2 <= 4e-3 over the whole tensor, max-abs <= 2^-6 |ref|_inf) passes the
same fault on the inputs the existing tests draw (one distribution for every sample, group and row).  The table, as printed
(all 18 mkd_groupnorm rows and all 18 LayerNorm shapes; "by" = the smallest worst err / bound over the rows):

  mutant                      over the bound (hard set)                  the global check passes it (iid inputs)
  drop_last_pixel             18 of 18 rows, by >= 40 x                  on 8 of 18 rows: every row with hw >= 205
  double_last_pixel           18 of 18, by >= 40 x                       on 8 of 18: the same rows
  stats_of_previous_group     18 of 18, by >= 3.4e5 x                    on 0 of 18
  stats_of_previous_sample    15 of 15 (the rows with B = 2), 4.3e5 x    on 0 of 15
  affine_off_by_a_vector      18 of 18, by >= 1.3e4 x                    on 0 of 18
  no_silu_on_last_pixel       12 of 12 (the SiLU rows), by >= 1.1e4 x    on 0 of 12
  rstd_one                    18 of 18, by >= 2.3e4 x                    on 0 of 18
  mean_of_previous_row (LN)   18 of 18, by >= 5.3e4 x                    on 0 of 18
  drop_last_vector (LN)       18 of 18, by >= 5.6e3 x                    on 2 of 18 (5 x 1600, 37 x 2048)
At these shapes the global check still sees every fault that moves whole groups, rows or channels; it is blind to one pixel left out of, or
counted twice in, a group's statistics from hw = 205 on (what a ragged-tail mask, a clamped re-read or an unrolled tail can get wrong),
and to a LayerNorm row's last vector at the widest rows.  The per-element bound on the hard set sees each of them on every row, by a
factor of 40 at the least.  (Statistics of the wrong group or sample pass no row here even on iid inputs: the sampling noise between two
groups of one distribution is already several bf16 steps.)"""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R
from tests.gpu_util import assert_close_bf16

GN_IDS = [R.gn_id(c) for c in R.GN_CASES]
LN_SHAPES = [(rows, d) for rows in R.LN_ROWS for d in R.LN_D]
_cache = {}


def gn_data(name, c):
    """(x, gamma, beta, ref, bound) of one (set, row), computed once."""
    key = ('gn', name, c)
    if key not in _cache:
        x = R.gn_input(name, c.B, c.hw, c.C)
        gamma, beta = R.affine(c.C, 0)
        _cache[key] = (x, gamma, beta) + R.gn_ref(x, gamma, beta, c.eps, c.silu)
    return _cache[key]


def ln_data(name, rows, d):
    key = ('ln', name, rows, d)
    if key not in _cache:
        x = R.ln_input(name, rows, d)
        gamma, beta = R.affine(d, 1)
        _cache[key] = (x, gamma, beta) + R.ln_ref(x, gamma, beta, 1e-5)
    return _cache[key]


def global_check_passes(out, want):
    try:
        assert_close_bf16(out, want)
    except AssertionError:
        return False
    return True


def test_shape_tables_reach_every_branch():
    got = {}
    for c in R.GN_CASES:
        got.setdefault(R.branch_of(c.hw, c.C), []).append(R.gn_id(c))
    for br, ids in sorted(got.items(), key=str):
        print(f'{tuple(br)}: {", ".join(ids)}')
    assert set(got) == R.GN_BRANCHES, f'missing {R.GN_BRANCHES - set(got)}, unexpected {set(got) - R.GN_BRANCHES}'
    # what the issue's table says of single rows
    br = {(c.C, c.hw): R.branch_of(c.hw, c.C) for c in R.GN_CASES}
    assert br[320, 16] == ('fused', 256, 4, 'register') and br[320, 205] == ('fused', 256, 8, 'register')
    assert br[320, 409] == ('fused', 256, 16, 'register') and br[320, 817] == ('fused', 512, 16, 'register')
    assert br[320, 1633] == ('fused', 256, 0, 'register') and br[2560, 101] == ('fused', 256, 8, 'register')
    assert br[192, 100] == ('fused', 256, 4, 'lds_tree') and br[192, 2724] == ('fused', 1024, 8, 'lds_tree')
    assert br[192, 3000] == ('fused', 256, 0, 'lds_tree')
    assert br[960, 1640] == br[192, 8200] == ('two_kernel', 240, None, 'partials')
    cgs = {c.C // R.GROUPS for c in R.GN_CASES if R.branch_of(c.hw, c.C).kernel == 'two_kernel'}
    assert min(cgs) < 8 <= max(cgs), 'the two-kernel path needs a row with cg < 8 and one with cg >= 8'
    # geometry the rows were chosen for
    g = R.gn_geometry(1633, 320)
    assert g.P == 51 and 1633 % (4 * g.P) == 1                      # streaming: 8 rounds of the 4-way loop, then one row for lane 0 alone
    assert R.gn_geometry(100, 192).P == 85                          # the tree over a lane count that is no power of two
    g = R.gn_geometry(1640, 960)
    assert (g.nchunks, g.rows_per_chunk) == (64, 26) and 1640 - 63 * 26 == 2          # a last chunk of 2 rows
    assert any(c.pad for c in R.GN_CASES) and {c.silu for c in R.GN_CASES} == {0, 1} and {c.eps for c in R.GN_CASES} == {1e-5, 1e-6}
    assert {c.hw % 2 for c in R.GN_CASES} == {0, 1}
    # gn_slab_kernel: NV 4, 8, 16
    assert [R.slab_branch_of(c.H * c.W, R.SLAB_COUT) for c in R.SLAB_CASES] == [('slab', 256, 4, 'register'), ('slab', 256, 8, 'register'),
                                                                                 ('slab', 512, 16, 'register')]
    # LayerNorm
    ln = {}
    for d in R.LN_D:
        ln.setdefault(R.ln_branch_of(d), []).append(d)
    assert set(ln) == R.LN_BRANCHES, f'missing {R.LN_BRANCHES - set(ln)}'
    assert all(R.ln_branch_of(d) == rc for d, rc in R.LN_ERRORS.items())


@pytest.mark.parametrize('drop', range(len(R.GN_CASES)))
def test_no_row_of_the_groupnorm_table_is_spare_without_notice(drop):
    """Taking a row away must either leave every branch with a shape, or be noticed: the coverage above is an assertion."""
    rest = [c for i, c in enumerate(R.GN_CASES) if i != drop]
    only = [br for br in R.GN_BRANCHES if not any(R.branch_of(c.hw, c.C) == br for c in rest)]
    sole = sum(R.branch_of(c.hw, c.C) == R.branch_of(R.GN_CASES[drop].hw, R.GN_CASES[drop].C) for c in R.GN_CASES) == 1
    assert bool(only) == sole


def test_every_chain_of_additions_is_below_k():
    for c in R.GN_CASES:
        n = R.gn_chain(c.hw, c.C)
        print(f'{R.gn_id(c)}: {tuple(R.branch_of(c.hw, c.C))} chain {n}')
        assert n <= R.K_GN, R.gn_id(c)
    assert R.gn_chain(1640, 960) == R.gn_chain(8200, 192) == 13 + 60 + 64
    for c in R.STAT_CASES:
        for ncols in (c.split, c.C - c.split):
            P, rpb, blocks = R.stat_colstats_geometry(c, ncols)
            assert rpb // P <= 16 and c.C % 32 == 0 and ncols % 8 == 0
    assert all(8 * nv + 6 <= R.K_LN for nv, _ in R.LN_BRANCHES)


def test_split_statistics_shapes():
    by = {(c.C, c.hw): c for c in R.STAT_CASES}
    assert {c.C for c in R.STAT_CASES} == {64, 320, 1280, 2560}
    c = by[320, 100]
    assert c.B == 2 and R.stat_apply_geometry(c)[2] > 1 and c.hw % R.stat_apply_geometry(c)[1]          # several blocks, a ragged last one
    for ncols in (c.split, c.C - c.split):
        P, rpb, blocks = R.stat_colstats_geometry(c, ncols)
        assert blocks > 1 and c.hw % rpb
    P, rpb, blocks = R.stat_apply_geometry(by[1280, 1100])
    assert 4 * P < rpb < 8 * P and rpb % (4 * P) and blocks > 1          # the 4-deep prefetch loop runs twice, the second time ragged
    assert R.stat_thread_shape(2560) == (320, 1)
    assert sum('degenerate' in c.sets for c in R.STAT_CASES) == 1 and all('hard' in c.sets for c in R.STAT_CASES)


@pytest.mark.parametrize('name', R.GN_SETS)
def test_groupnorm_inputs(name):
    B, hw, C = 2, 100, 320
    x = R.gn_input(name, B, hw, C)
    assert torch.equal(R.q16(x), x)
    xg = x.double().view(B, hw, R.GROUPS, -1)
    mu, sd = xg[:, 1:-1].mean((1, 3)), xg[:, 1:-1].std((1, 3))          # (of the pixels between the two shifted ones)
    live = torch.ones(B, R.GROUPS, dtype=torch.bool)
    if name == 'degenerate':
        for b in range(B):
            z, c3, c100 = R.degenerate_groups(b)
            assert (xg[b, :, z] == 0).all() and (xg[b, :, c3] == 3).all() and (xg[b, :, c100] == -100).all()
            live[b, [z, c3, c100]] = False
        assert len({R.degenerate_groups(b) for b in range(B)}) == B and not set(R.degenerate_groups(0)) & set(R.degenerate_groups(1))
    ratio = (mu.abs() / sd)[live]
    lim = {'hard': 4, 'degenerate': 4, 'offset': 16, 'far': 100}[name]
    assert lim * 0.8 <= ratio.max() <= lim * 1.1          # (sampling noise and the bf16 rounding of the values)
    assert sd[live].max() / sd[live].min() > 12                      # standard deviations from 1/4 to 4
    # pixel 0 high, the last pixel low, by about six standard deviations of their group
    assert (((xg[:, 0].mean(2) - mu) / sd)[live] > 4.5).all() and (((xg[:, -1].mean(2) - mu) / sd)[live] < -4.5).all()


def test_layernorm_inputs():
    for name in R.LN_SETS:
        x = R.ln_input(name, 37, 640)
        assert torch.equal(R.q16(x), x)
        mu, sd = x[:, 8:-8].double().mean(1), x[:, 8:-8].double().std(1)          # (of the channels between the shifted ones)
        assert (x[:, :8].double().mean(1) - mu > 4 * sd).all() and (x[:, -8:].double().mean(1) - mu < -4 * sd).all()
        if name == 'offset':
            assert mu.max() > 45 and mu.min() < -45 and mu.abs().max() <= 51


@pytest.mark.parametrize('c', R.GN_CASES[:6] + R.GN_CASES[11:14], ids=GN_IDS[:6] + GN_IDS[11:14])
def test_groupnorm_reference_is_torch_group_norm(c):
    x, gamma, beta, ref, bnd = gn_data('hard', c)
    want = F.group_norm(x.double().permute(0, 2, 1), R.GROUPS, gamma.double(), beta.double(), c.eps)
    want = (F.silu(want) if c.silu else want).permute(0, 2, 1)
    assert (ref - want).abs().max() <= 1e-9 * max(1.0, float(want.abs().max())) and (bnd > 0).all() and torch.isfinite(bnd).all()


def test_layernorm_reference_is_torch_layer_norm():
    for rows, d in LN_SHAPES[:4]:
        x, gamma, beta, ref, bnd = ln_data('offset', rows, d)
        want = F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5)
        assert (ref - want).abs().max() <= 1e-9 * float(want.abs().max()) and (bnd > 0).all()


def test_degenerate_groups_have_beta_as_reference_and_a_finite_bound():
    c = next(c for c in R.GN_CASES if (c.C, c.hw) == (320, 205))
    x, gamma, beta, ref, bnd = gn_data('degenerate', c)
    cg = c.C // R.GROUPS
    for b in range(c.B):
        for gidx in R.degenerate_groups(b):
            sl = slice(gidx * cg, (gidx + 1) * cg)
            assert torch.equal(ref[b, :, sl], beta[sl].double().expand(c.hw, cg)) and torch.isfinite(bnd[b, :, sl]).all()


@pytest.mark.parametrize('c', R.GN_CASES, ids=GN_IDS)
def test_correct_groupnorm_emulation_is_within_the_bound(c):
    for name in c.sets:
        x, gamma, beta, ref, bnd = gn_data(name, c)
        for order in ('chunked', 'sequential'):
            r = R.ratios(R.gn_emulate(x, gamma, beta, c.eps, c.silu, order=order), ref, bnd)
            i = int(r.argmax())
            print(f'emulation {R.gn_id(c)} {name} {order}: worst err / bound {r.max():.3f} at {R.locate(c.hw, c.C, i // (c.hw * c.C), i // c.C % c.hw, i % c.C)}')
            assert r.max() <= 1.0, f'{R.gn_id(c)} {name} {order}: {r.max():.3f}'
    x, gamma, beta, ref, _ = gn_data('iid', c)
    assert global_check_passes(R.gn_emulate(x, gamma, beta, c.eps, c.silu), ref)


@pytest.mark.parametrize('rows,d', LN_SHAPES)
def test_correct_layernorm_emulation_is_within_the_bound(rows, d):
    for name in R.LN_SETS:
        x, gamma, beta, ref, bnd = ln_data(name, rows, d)
        for order in ('chunked', 'sequential'):
            r = R.ratios(R.ln_emulate(x, gamma, beta, 1e-5, order=order), ref, bnd)
            print(f'emulation LN {rows}x{d} {name} {order}: worst err / bound {r.max():.3f}')
            assert r.max() <= 1.0, f'{rows}x{d} {name} {order}: {r.max():.3f}'


def test_every_mutant_is_flagged_on_every_row():
    lines = []
    for mutant in R.GN_MUTANTS:
        worst, old = [], []
        for c in R.GN_CASES:
            if not R.gn_applies(mutant, c.B, c.silu):
                continue
            x, gamma, beta, ref, bnd = gn_data('hard', c)
            worst.append((float(R.ratios(R.gn_emulate(x, gamma, beta, c.eps, c.silu, mutant=mutant), ref, bnd).max()), R.gn_id(c)))
            x, gamma, beta, ref, bnd = gn_data('iid', c)
            old.append((R.gn_id(c), global_check_passes(R.gn_emulate(x, gamma, beta, c.eps, c.silu, mutant=mutant), ref)))
        lines.append((mutant, worst, old))
    for mutant in R.LN_MUTANTS:
        worst, old = [], []
        for rows, d in LN_SHAPES:
            x, gamma, beta, ref, bnd = ln_data('hard', rows, d)
            worst.append((float(R.ratios(R.ln_emulate(x, gamma, beta, 1e-5, mutant=mutant), ref, bnd).max()), f'{rows}x{d}'))
            x, gamma, beta, ref, bnd = ln_data('iid', rows, d)
            old.append((f'{rows}x{d}', global_check_passes(R.ln_emulate(x, gamma, beta, 1e-5, mutant=mutant), ref)))
        lines.append((mutant, worst, old))
    for mutant, worst, old in lines:
        passed = [i for i, p in old if p]
        print(f'MUTANT {mutant}: over the bound on {sum(w > 1 for w, _ in worst)} of {len(worst)} rows (smallest worst err / bound '
              f'{min(worst)[0]:.1f} at {min(worst)[1]}); the global check passes it on {len(passed)} of {len(old)} rows (iid inputs)')
        if passed and len(passed) < len(old):
            print('    passes: ' + ' '.join(passed))
    for mutant, worst, old in lines:
        assert all(w > 1 for w, _ in worst), f'{mutant}: not flagged on {[i for w, i in worst if not w > 1]}'
    table = {m: [p for _, p in old] for m, _, old in lines}
    # the record of what the per-element tests add: the global check lets these through somewhere
    for mutant in ('drop_last_pixel', 'double_last_pixel', 'drop_last_vector'):
        assert any(table[mutant]), f'{mutant}: the global check catches it on every row'
