"""No GPU: the cases and input sets of tests/test_gpu_gemm_elements.py satisfy the conditions its tests rely on (the exact sets are
exact in bf16, every LDS-staged row takes at least two geometries, the float64 reference agrees with torch's conv2d), a correct fp32
emulation of the kernels stays within the per-element bound of tests/gemm_ref.py on every case and set and is bit-equal on the exact
ones, and every emulation that is wrong on purpose is flagged by some set on some case.  The table printed by
test_every_mutant_is_flagged also says, per mutant, whether the suite's global check (assert_close_bf16: rel-L2 <= 4e-3 over the whole
tensor, max-abs <= 2^-6 |ref|_inf) would have passed it: that is the record of what the per-element tests add."""
import pytest
import torch
import torch.nn.functional as F

from makeupdiffuse_amd import lib as mlib
from tests import gemm_ref as R
from tests.gpu_util import assert_close_bf16

ROWS = R.tile_rows(mlib.tile_table())
CASES = R.cases()
IDS = [c.id for c in CASES]
_cache = {}


def supported(row, c):
    cv = c.conv
    return mlib.load().mkd_gemm_cfg_supported(row.index, c.M, c.N, c.K, 1, cv.H, cv.W, cv.Cin, cv.Hout, cv.Wout, cv.stride, cv.up) == 1


def data(name, c):
    """(inputs, y, z, S, bound) of one (set, case), computed once."""
    if (name, c.id) not in _cache:
        d = R.build(name, c)
        _cache[name, c.id] = (d,) + R.ref(c, d)
    return _cache[name, c.id]


def global_check_passes(out, want):
    try:
        assert_close_bf16(out, want)
    except AssertionError:
        return False
    return True


def test_tile_table_and_case_list():
    assert len(set(IDS)) == len(IDS)
    fams = {r.family for r in ROWS}
    assert fams == {'GEMM', 'KSPLIT', 'LIGHT', 'PATCH', 'RA'}
    for r in ROWS:
        assert r.TM % (16 * r.WM) == 0 and r.TN % (16 * r.WN) == 0 and (r.KW == 1) == (r.family != 'KSPLIT')
        assert R.folds_second_input(r) == (r.family in ('GEMM', 'KSPLIT', 'LIGHT'))
    # the shapes the launcher accepts, and the K-step counts the linear cases put against every ring depth and K-group count
    for c in CASES:
        assert c.N % 4 == 0 and c.K % 8 == 0 and c.lda % 8 == 0 and c.ldw % 8 == 0 and c.ldn % 4 == 0 and c.ldx2 % 8 == 0, c.id
        assert c.M <= (520 if c.kind == 'linear' else 1024) and c.N <= 324 and c.K <= 1344, c.id          # (quick: nothing larger)
        assert R.case_rows(c, ROWS, supported), c.id
    steps = {-(-c.K // R.BK) for c in CASES if c.kind == 'linear'}
    assert steps >= {1, 2, 3, 4, 6, 8, 21}
    assert max(r.STAGES for r in ROWS) == 6 and max(r.KW for r in ROWS) == 4
    assert any(c.N % 16 and c.N % 4 == 0 for c in CASES) and any(c.ldw > c.K for c in CASES) and any(c.kind == 'linear' and c.lda > c.K for c in CASES)
    assert any(c.splitk > len(R.slabs(c)) and len(R.slabs(c)) == -(-c.K // R.BK) for c in CASES)          # a request above the K-step count
    assert any(len(R.slabs(c)[-1]) < len(R.slabs(c)[0]) or R.slabs(c)[-1][-1][1] - R.slabs(c)[-1][-1][0] < R.BK for c in CASES if len(R.slabs(c)) > 1)


def test_every_lds_staged_row_takes_at_least_two_geometries():
    geos = [c for c in CASES if c.kind == 'patch']
    assert len(geos) == 4
    for r in ROWS:
        if r.family == 'PATCH':
            took = [c.id for c in geos if supported(r, c)]
            print(f'row {r.index} {r.name}: {", ".join(took)}')
            assert len(took) >= 2, f'row {r.index} {r.name} takes only {took}'
        else:
            assert not any(r in R.case_rows(c, ROWS, supported) for c in geos)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_builder_properties(c):
    for name in R.sets_of(c):
        d, y, z, S, bnd = data(name, c)
        for k, v in d.items():
            if torch.is_tensor(v):
                assert R.is_bf16(v), f'{c.id} {name}: {k} is not bf16'
        assert y.shape == (c.M, c.N // 2 if c.act == 2 else c.N) and torch.isfinite(y).all() and (bnd > 0).all()
        assert (S >= z.abs() - 1e-9).all()
        if R.bit_exact(name, c):          # a condition, not a skip: the expected values themselves are bf16 numbers
            assert R.is_bf16(y), f'{c.id} {name}: |y| up to {y.abs().max():.1f} is not exact in bf16'
            assert float(S.max()) < 2 ** 24          # ... and every fp32 partial sum, in any order, is an exact integer multiple of 2^-4
        if name == 'ones':
            cv = c.conv
            taps = R.gather(c, d['x'], d['x2'])[:, :9 * cv.Cin].sum(1) / cv.Cin          # taps inside the image, per output pixel
            assert taps.min() < 9 and taps.max() == 9 and set(taps.tolist()) <= {4.0, 6.0, 9.0}
    assert ('exact' in R.sets_of(c)) == (c.act in (0, 4)) and ('ones' in R.sets_of(c)) == (c.conv is not None)


@pytest.mark.parametrize('c', [c for c in CASES if c.conv is not None], ids=[c.id for c in CASES if c.conv is not None])
def test_conv_reference_is_torch_conv2d(c):
    cv = c.conv
    d, y, z, S, _ = data('randn', c)
    x = d['x'].double().permute(0, 3, 1, 2)
    if cv.up:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if cv.pad_tl == 0:
        x = F.pad(x, (0, 1, 0, 1))
    w = d['w'].double()[:, :9 * cv.Cin].reshape(c.N, 3, 3, cv.Cin).permute(0, 3, 1, 2)
    want = F.conv2d(x, w, d['bias'].double(), stride=cv.stride, padding=1 if cv.pad_tl else 0)
    assert want.shape[2:] == (cv.Hout, cv.Wout)
    want = want.permute(0, 2, 3, 1).reshape(c.M, c.N)
    if cv.K2:
        want = want + d['x2'].double() @ d['w'].double()[:, 9 * cv.Cin:].t()
    if c.rpb:
        want = want + d['rowbias'].double().repeat_interleave(c.rpb, 0)[:c.M]
    if c.res:
        want = want + d['R'].double()
    assert (y - want).abs().max() <= 1e-11 * max(1.0, float(S.max()))


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_correct_emulation_is_within_the_bound_on_every_set(c):
    for name in R.sets_of(c):
        d, y, z, S, bnd = data(name, c)
        out = R.emulate(c, d)
        r = R.ratios(out, y, bnd)
        line, fail = R.report(R.case_rows(c, ROWS, supported)[0], c, name, r)
        print(line.replace('GEMMEL', 'emulation'))
        assert fail is None, f'{c.id} {fail}'
        # (<= 1, not the 0.98 a handful of shapes may suggest: round-to-nearest moves y = 2^e (1 + 2^-8 + tiny) by half a unit in the last
        # place, 2^(e - 8) = |y| 2^-8 / (1 + 2^-8): a CORRECT kernel reaches 0.996 of the rounding term alone, and with 6144 elements at
        # K = 8 this emulation is at 0.992)
        assert r.max() <= 1.0
        if R.bit_exact(name, c):
            assert torch.equal(out.double(), y), f'{c.id} {name}: the correct emulation is not bit-equal'
        if name == 'randn':
            assert global_check_passes(out, y)


def flagged(name, c, out, y, bnd):
    if R.bit_exact(name, c):
        return not torch.equal(out.double(), y)
    return not bool((R.ratios(out, y, bnd) <= 1.0).all())


def test_every_mutant_is_flagged():
    """Per mutant: which (set, case) flags it, and whether the global check would have passed it there (randn: the set it runs on)."""
    table = {}
    for mutant in R.MUTANTS:
        hits, passes_old = [], []
        for c in CASES:
            if not R.applies(mutant, c):
                continue
            for name in R.sets_of(c):
                d, y, z, S, bnd = data(name, c)
                out = R.emulate(c, d, mutant)
                if flagged(name, c, out, y, bnd):
                    hits.append((name, c.id))
                if name == 'randn':
                    passes_old.append((c.id, global_check_passes(out, y)))
        table[mutant] = (hits, passes_old)
    for mutant, (hits, old) in table.items():
        by_set = {s: sum(1 for n, _ in hits if n == s) for s in R.SETS}
        print(f'MUTANT {mutant}: flagged by ' + ', '.join(f'{s} on {k} cases' for s, k in by_set.items() if k) +
              f'; the global check passes it on {sum(p for _, p in old)} of {len(old)} cases (randn)')
        if len(hits) <= 8:
            print('    ' + ' '.join(f'{n}:{cid}' for n, cid in hits))
    for mutant, (hits, old) in table.items():
        assert hits, f'{mutant}: no set flags it on any case'
    # the sets do what they were built for: one dropped chunk needs the exact set at K = 1344; a padding fault shows on ones
    assert ('exact', 'L520x320x1344') in table['drop_chunk'][0] and ('exact', 'L520x320x1344') in table['drop_product'][0]
    assert any(n == 'ones' for n, _ in table['zero_tap'][0]) and any(n == 'ones' for n, _ in table['halo_neighbour'][0])
    assert any(n == 'randn' for n, _ in table['truncate'][0])
    # ... and the global check lets most of them through somewhere
    for mutant in ('drop_product', 'truncate', 'residual_after_round'):
        assert any(p for _, p in table[mutant][1]), f'{mutant}: the global check catches it everywhere'


def test_locate_names_tile_wave_and_fragment():
    by_name = {r.name: r for r in ROWS}
    c = next(c for c in CASES if c.id == 'L520x320x1344')
    r = by_name['256x128']                       # 4 x 2 waves of 64 x 64
    assert (r.TM, r.TN, r.WM, r.WN) == (256, 128, 4, 2)
    assert R.locate(r, c, 0, 0) == 'tile (0, 0) wave (0, 0) fragment (0, 0)'
    assert R.locate(r, c, 519, 319) == 'tile (2, 2) wave (0, 0) fragment (0, 3)'
    assert R.locate(r, c, 256 + 64 + 17, 128 + 63) == 'tile (1, 1) wave (1, 0) fragment (1, 3)'
    r = by_name['ra128x160']                     # 4 waves of 32 rows, all 160 columns
    assert (r.TM, r.TN, r.WM, r.WN) == (128, 160, 4, 1)
    assert R.locate(r, c, 519, 319) == 'tile (4, 1) wave (0, 0) fragment (0, 9)'
    assert R.locate(r, c, 127, 159) == 'tile (0, 0) wave (3, 0) fragment (1, 9)'
    # an LDS-staged row: B2 16 x 32 on 128-pixel tiles of 8 x 16: pixel (b 1, y 9, x 20) is row 4 of the tile's second image row
    c = next(c for c in CASES if c.id == 'P-B2-16x32-c64-32')
    r = by_name['patch128x64']
    assert R.patch_geometry(r, c) == (8, 16, 1)
    assert R.locate(r, c, 512 + 9 * 32 + 20, 31) == 'tile (7, 0) wave (0, 0) fragment (1, 1)'
