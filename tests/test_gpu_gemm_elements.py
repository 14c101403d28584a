"""-m gpu: the implicit-GEMM family (gemm_kernel, gemm_ra_kernel, conv3x3_patch_kernel and the split-K reduce kernels: csrc/kernels_gemm.hip,
kernels_conv.hip) through mkd_gemm_bf16 / mkd_gemm_gnstat_bf16 / mkd_conv3x3_down_bf16 / mkd_conv3x3_fold_bf16, per output ELEMENT, on
every row of the tile table (csrc/gemm_tiles.inc, enumerated through mkd_gemm_tile_info and forced with mkd_gemm_force_tile).  One test is
one case of tests/gemm_ref.py: cases() on one row, with all of its input sets:
  randn   |out - y| <= the derived per-element bound (gemm_ref.py: 2^-8 |y| + (K + 4) 2^-23 S, propagated through the activations),
          against a float64 CPU reference on the bf16-rounded inputs; and the suite's global check (assert_close_bf16)
  exact   A, W in {-1, 0, 1}, small-integer bias / row bias / residual: every expected value is a bf16 number, every element is compared
          BIT FOR BIT (one missing or duplicated product at any K)
  ones    (conv) x = 1, w = 1/8: y counts the taps inside the image, a halo or padding fault is an exact integer difference
A, W, R, the row bias and C sit in NaN-filled buffers at the case's strides; C is followed by 128 guard rows.  Every launch runs twice:
bit-repeatable, finite inside M x N, NaN in every gap column and guard row.  A failure names element, tile, wave and fragment.

Measured on MI355X, worst err / bound over the cases and rows of a family (median of the per-(case, row) worst in brackets); the
bit-exact sets: (case, row) runs, every element equal in every one:
  GEMM    randn 0.992 (0.940), from K = 136 on 0.968, fp32 output 0.0050      exact 210 runs, ones 84 runs: equal
  KSPLIT  randn 0.992 (0.940), from K = 136 on 0.968, fp32 output 0.0030      exact 140 runs, ones 60 runs: equal
  LIGHT   randn 0.992 (0.940), from K = 136 on 0.968, fp32 output 0.0050      exact 140 runs, ones 60 runs: equal
  RA      randn 0.992 (0.941), from K = 136 on 0.968, fp32 output 0.0050      exact  78 runs, ones 30 runs: equal
  PATCH   randn 0.934 (0.890)                                                 exact  40 runs, ones 40 runs: equal
The worst anywhere is 0.992 (L96x64x8, element (78, 46), on every row): the CPU emulation of a correct kernel has the same 0.992 at the
same element - a value just above a power of two that the bf16 rounding moves by nearly half a unit in the last place; from K = 136 on
the worst is 0.968 (G-B2-7x5-c24-132-s2), as on the CPU.  With fp32 output the kernels use 0.5 % of the bound: the accumulation term is
wide (any order, truncating adders allowed) and the matrix cores are far inside it.  No case on any row found a fault.

What the per-element checks add, from tests/test_gemm_ref_host.py::test_every_mutant_is_flagged (CPU emulations that are wrong on
purpose; "global" = assert_close_bf16 on the randn set of the same cases):
  mutant                 flagged by (cases)                       global check passes it on
  drop_product           exact 18, randn 16 (fp32 output, small K), ones 5     24 of 24 cases
  drop_chunk             randn 24, exact 19, ones 10               0 of 24 (K <= 1344 here)
  zero_tap               randn 10, exact 10, ones 10               0 of 10
  halo_neighbour         randn 8, exact 8, ones 8                  0 of 8
  truncate               randn 22                                  22 of 22
  residual_after_round   randn 4                                   4 of 4
  rowbias_of_wave        randn 6, exact 5, ones 2                  0 of 6
  skip_bias_tail         randn 24, exact 19, ones 10               0 of 24
  drop_last_slab         randn 5, exact 3, ones 2                  0 of 5
At these (quick) shapes the global check still sees every fault that moves an element by a good part of a unit; it is blind to one missing
product, to truncation and to a residual added after the rounding, on every case, and those are what the bound and the exact set catch.
The any-order fp32 term grows like K S: at K = 11520 (CPU emulation, 64 x 64) a dropped chunk reaches only 0.77 of the bound on randn, so
at any K it is the exact set that answers for single products and chunks, and the bound for the rounding and the epilogue."""
import ctypes as C

import pytest
import torch

from makeupdiffuse_amd import lib as mlib
from tests import gemm_ref as R
from tests.gpu_util import DEV, L, assert_close_bf16, sync

pytestmark = pytest.mark.gpu

ROWS = R.tile_rows(mlib.tile_table())
NAN = float('nan')
GUARD = 128
_host, _dev = {}, {}


def supported(row, c):
    cv = c.conv
    return mlib.load().mkd_gemm_cfg_supported(row.index, c.M, c.N, c.K, 1, cv.H, cv.W, cv.Cin, cv.Hout, cv.Wout, cv.stride, cv.up) == 1


PAIRS = [(c, r) for c in R.cases() for r in R.case_rows(c, ROWS, supported)]


def padded(x, ld, dtype=torch.bfloat16):
    """x [rows, n] in the first columns of a NaN-filled [rows, ld] device buffer."""
    rows, n = x.shape
    buf = torch.full((rows, ld), NAN, dtype=dtype)
    buf[:, :n] = x.to(dtype)
    return buf.to(DEV)


def host(name, c):
    """(inputs, y, bound) of one (set, case): computed once, shared by every row, never changed."""
    if (name, c.id) not in _host:
        d = R.build(name, c)
        y, _, _, bnd = R.ref(c, d)
        _host[name, c.id] = (d, y, bnd)
    return _host[name, c.id]


def device(name, c):
    if (name, c.id) not in _dev:
        d = host(name, c)[0]
        x = d['x'].reshape(-1, d['x'].shape[-1])
        _dev[name, c.id] = dict(
            x=padded(x, c.lda), w=padded(d['w'], c.ldw), x2=None if d['x2'] is None else padded(d['x2'], c.ldx2),
            bias=None if d['bias'] is None else d['bias'].to(DEV),
            rowbias=None if d['rowbias'] is None else padded(d['rowbias'], c.ldn, torch.float32),          # EXACTLY the samples' rows
            R=None if d['R'] is None else padded(d['R'], c.ldn))
    return _dev[name, c.id]


def ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def launch(c, b, scale, out, gn):
    cv = c.conv
    if c.entry == 'down':
        return L().mkd_conv3x3_down_bf16(ptr(b['x']), c.lda, ptr(b['w']), ptr(b['bias']), ptr(out), c.ldn, cv.B, cv.H, cv.W, cv.Cin, c.N, c.splitk, None)
    if c.entry == 'fold':
        return L().mkd_conv3x3_fold_bf16(ptr(b['x']), c.lda, ptr(b['w']), ptr(b['bias']), ptr(b['x2']), c.ldx2, cv.K2, ptr(out), c.ldn,
                                         cv.B, cv.H, cv.W, cv.Cin, c.N, c.splitk, None)
    geo = (0, 0, 0, 0, 0, 0, 0, 1, 0) if cv is None else (1, cv.B, cv.H, cv.W, cv.Cin, cv.Hout, cv.Wout, cv.stride, cv.up)
    args = (ptr(b['x']), c.lda, ptr(b['w']), c.ldw, ptr(b['bias']), ptr(b['rowbias']), c.ldn if c.rpb else 0, c.rpb if c.rpb else 1,
            ptr(b['R']), c.ldn if c.res else 0, scale, c.act, ptr(out), c.ldn, int(c.f32), c.M, c.N, c.K, *geo, c.splitk)
    if c.entry == 'gnstat':          # 12 channels per group, one sample per row-bias sample; the statistics keep their own test
        gn.zero_()
        return L().mkd_gemm_gnstat_bf16(*args, ptr(gn), 12, 0, c.rpb, None)
    return L().mkd_gemm_bf16(*args, None)


def run(c, name):
    """Two launches into a NaN-filled C [M + 128, ldn]: bit-repeatable, finite inside, NaN outside.  Returns [M, N'] fp32."""
    d = host(name, c)[0]
    b = device(name, c)
    ncol = c.N // 2 if c.act == 2 else c.N
    out = torch.empty((c.M + GUARD, c.ldn), device=DEV, dtype=torch.float32 if c.f32 else torch.bfloat16)
    gn = torch.zeros((-(-c.M // c.rpb), 32, 2), device=DEV, dtype=torch.int64) if c.entry == 'gnstat' else None

    def once():
        out.fill_(NAN)
        rc = launch(c, b, float(d['scale']), out, gn)
        assert rc == 0, L().mkd_last_error()
        sync()
        return out.cpu()

    first, second = once(), once()
    bits = torch.int32 if c.f32 else torch.int16
    assert torch.equal(first.view(bits), second.view(bits)), f'{name}: not bit-repeatable'
    res = second[:c.M, :ncol].float()
    assert torch.isfinite(res).all(), f'{name}: non-finite output'
    assert torch.isnan(second[:c.M, ncol:].float()).all() and torch.isnan(second[c.M:].float()).all(), f'{name}: wrote outside its rows / columns'
    return res


@pytest.mark.parametrize('c,row', PAIRS, ids=[f'{c.id}-{r.name}' for c, r in PAIRS])
def test_gemm_elements(c, row):
    failures = []
    L().mkd_gemm_force_tile(row.index)
    try:
        for name in R.sets_of(c):
            d, y, bnd = host(name, c)
            out = run(c, name)
            if R.bit_exact(name, c):
                diff = out.double() != y
                bad = int(diff.sum())
                print(f'GEMMEL {row.family} {name} {c.id} row {row.index} {row.name}: {bad} of {y.numel()} elements differ')
                if bad:
                    m, n = divmod(int(diff.flatten().nonzero()[0]), y.shape[1])
                    worst = (out.double() - y).abs().max()
                    failures.append(f'{name}: {bad} elements are not bit-equal (largest difference {worst:g}), the first ({m}, {n}): '
                                    f'{out[m, n]:g} for {y[m, n]:g}, {R.locate(row, c, m, n)}')
            else:
                line, fail = R.report(row, c, name, R.ratios(out, y, bnd))
                print(line)
                if fail:
                    failures.append(fail)
            if name == 'randn':
                assert_close_bf16(out, y, what=f'{c.id} row {row.index}')
    finally:
        L().mkd_gemm_force_tile(-1)
    assert not failures, f'{c.id} on row {row.index} {row.name}: ' + '; '.join(failures)


def test_one_changed_weight_shows_in_its_column_alone():
    """The comparison itself, end to end on the device: one weight of the exact set at K = 1344 set to zero (one product missing from every
    element of column 7) makes exactly the elements of that column whose A entry is non-zero differ, by exactly that product."""
    c = next(c for c in R.cases() if c.id == 'L520x320x1344')
    d, y, _ = host('exact', c)
    n, k = 7, 700
    assert d['w'][n, k] != 0
    clean = device('exact', c)
    b = dict(clean, w=clean['w'].clone())
    b['w'][n, k] = 0
    out = torch.full((c.M, c.ldn), NAN, device=DEV, dtype=torch.bfloat16)
    assert launch(c, b, 1.0, out, None) == 0, L().mkd_last_error()
    sync()
    diff = out.cpu()[:, :c.N].double() - y
    want = torch.zeros_like(y)
    want[:, n] = -d['x'][:, k].double() * d['w'][n, k].double()
    assert (want[:, n] != 0).sum() > 500 and torch.equal(diff, want)


def test_tile_rows_are_the_librarys():
    n = L().mkd_gemm_tile_info(-1, None, None, None, None)
    assert n == len(ROWS) and {r.index for _, r in PAIRS} == set(range(n)), 'a row of the tile table runs no case'
