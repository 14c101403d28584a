"""-m gpu: the norm kernels (csrc/kernels_norm.hip) per output ELEMENT, through mkd_groupnorm (gn_fused_kernel<4 / 8 / 16 / 0>, gn_stats_kernel +
gn_apply_kernel), mkd_gn_colstats + mkd_gn_apply_stats, mkd_gemm_groupnorm_bf16 (gn_slab_kernel<4 / 8 / 16>) and mkd_layernorm /
mkd_layernorm_ld (layernorm_kernel<1 .. 4>), on the shape tables and input sets of tests/norm_ref.py: every (sample, group) and every
row with its own mean and scale, heavy values on the first and last pixel, constant and all-zero groups.  Every case puts its inputs at
their strides in NaN-filled buffers, gives the output a row stride wider than C (where the entry point takes one) and guard rows behind
it, launches twice and requires: bit-equal results; finite values inside the tensor, NaN in every gap column and guard row, the input
buffers bit-unchanged; |out - ref| <= the derived per-element bound of norm_ref.py against the float64 reference.  A failure names sample,
pixel, channel, group, block, the thread's vector and pixel lane, and the branch.  No case skips; -4 from a launcher is a failure.

Measured on MI355X, worst err / bound over the rows of each table (every run prints its own figure and where its worst element is
computed):
  mkd_groupnorm          hard 0.990 (2560 / 16), offset 0.988, degenerate 0.983 over 18 rows: fused<4> 0.990, fused<8> 0.989, fused<16> 0.987
                         (256 and 512 threads), fused<8> on 1024 threads 0.977, streaming 0.985 (registers) / 0.984 (tree), the LDS tree 0.988,
                         the two-kernel pair 0.987 (cg 30) / 0.981 (cg 6)
  colstats + apply       hard 0.990 (1280 / 1100, the second round of the prefetch loop), degenerate 0.987, exact 0.985; the all-zero group
                         is bf16(act(beta)) on every element with and without SiLU; the exact set's gstat equals the integer sums bit for bit
  gn_slab_kernel         0.978 / 0.981 / 0.988 at NV 4 / 8 / 16, bit-equal to split-K reduce + mkd_groupnorm
  layernorm_kernel       hard 0.992 (37 x 2048), offset 0.984 over 9 widths x 2 row counts x 3 input strides; the stride never changes a bit
Every worst element is one the bf16 rounding moves by nearly half a unit in the last place, as in the CPU emulation of a correct kernel
(0.99): the statistics terms of the bound are not what is used up.  On the constant groups (3.0 and -100: var = 0, E[x^2] - mean^2 is pure
cancellation clamped at 0) the largest |out - act(beta)| is 4.0e-3 (at -100, where x sa and mean sa are 3e4 and cancel) and at most 1e-3 on
the others.  No case on any branch found a fault.  With one pixel of 1640 changed under the kernel alone (960 / 1640), 35911 to 40465 of
the 49170 other elements of each group of that sample leave the bound and none of the other sample: the comparison sees one pixel.

The far set (|mean| / std = 100, no SiLU), per-(sample, group) rel-L2 against float64, worst (median):
                                   the kernel              torch F.group_norm on the device, bf16 in and out
  mkd_groupnorm 320 / 205          1.9e-3 (1.7e-3)         6.0e-2 (1.4e-2)
  mkd_groupnorm 960 / 1640         2.2e-3 (1.7e-3)         1.3e-2 (4.0e-3)
  colstats + apply 320 / 100       1.9e-3 (1.7e-3)         5.0e-2 (1.8e-2)
and 0.39 / 0.53 / 0.48 of the a-priori bound.  The kernels sit at the floor of the bf16 output rounding (a uniform rounding error is
2^-9 / sqrt 3 = 1.1e-3 relative at the top of a binade, up to twice that at its bottom) and below torch's own kernel: at this ratio the
one-pass variance from fp32 sums is not yet a limit of these kernels (its share of the bound, dv / var = 0.3, is a worst case over
orders of summation; chunked sums of <= 137 terms stay far inside it).

What the per-element checks add over the global check of test_groupnorm / test_layernorm: the table in tests/test_norm_ref_host.py.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R
from tests.gpu_util import DEV, L

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64
WIDER = 8          # the output's row stride is C + 8
_host = {}


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


def sync():
    torch.cuda.synchronize()


def strided(x, ld):
    """x [..., n] flattened to rows, in the first columns of a NaN-filled [rows, ld] bf16 device buffer."""
    x = x.reshape(-1, x.shape[-1])
    buf = torch.full((x.shape[0], ld), NAN, dtype=torch.bfloat16)
    buf[:, :x.shape[1]] = x.to(torch.bfloat16)
    return buf.to(DEV)


def twice(launch, outs, ins):
    """Run launch() twice into the NaN-filled buffers `outs`: return code 0, bit-repeatable, the input buffers `ins` bit-unchanged.
    Returns the CPU copies of outs."""
    before = [t.clone() for t in ins]
    res = []
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        rc = launch()
        assert rc == 0, f'launcher returned {rc}: {L().mkd_last_error()}'
        sync()
        res.append([o.cpu() for o in outs])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), 'not bit-repeatable'
    for t, b in zip(ins, before):
        view = torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64
        assert torch.equal(t.view(view), b.view(view)), 'an input buffer changed'
    return res[1]


def inside(buf, rows, n, what):
    """The [rows, n] tensor inside a [rows + GUARD, ld] buffer: finite there, NaN in every gap column and guard row."""
    t = buf[:rows, :n].float()
    assert torch.isfinite(t).all(), f'{what}: non-finite output'
    assert torch.isnan(buf[:rows, n:].float()).all() and torch.isnan(buf[rows:].float()).all(), f'{what}: wrote outside its rows / columns'
    return t


def gn_host(name, B, hw, C_, eps, silu):
    """(x, gamma, beta, ref, bound) of one (set, shape), computed once and never changed."""
    key = (name, B, hw, C_, eps, silu)
    if key not in _host:
        x = R.gn_input(name, B, hw, C_)
        gamma, beta = R.affine(C_, 0)
        _host[key] = (x, gamma, beta) + R.gn_ref(x, gamma, beta, eps, silu)
    return _host[key]


def torch_group_norm_error(x, gamma, beta, eps):
    """Per-(sample, group) rel-L2 of torch's own F.group_norm on the device, bf16 in and out (its affine parameters are bf16 then, and so
    are its reference's)."""
    gb, bb = R.q16(gamma), R.q16(beta)
    xd = x.to(DEV).to(torch.bfloat16).permute(0, 2, 1).contiguous()
    out = F.group_norm(xd, R.GROUPS, gb.to(DEV).to(torch.bfloat16), bb.to(DEV).to(torch.bfloat16), eps).permute(0, 2, 1).float().cpu()
    return R.group_rel_l2(out, R.gn_ref(x, gb, bb, eps, 0)[0])


def far_figures(tag, out, x, gamma, beta, eps, ref):
    ours, theirs = R.group_rel_l2(out, ref), torch_group_norm_error(x, gamma, beta, eps)
    print(f'NORMFAR {tag}: per-group rel-L2 against float64, worst (median): kernel {ours.max():.3e} ({ours.median():.3e}), '
          f'torch F.group_norm bf16 {theirs.max():.3e} ({theirs.median():.3e})')


# ---- mkd_groupnorm ---------------------------------------------------------------------------------------------------------------------------
def run_groupnorm(c, name, silu):
    x, gamma, beta, ref, bnd = gn_host(name, c.B, c.hw, c.C, c.eps, silu)
    xb = strided(x, c.C + c.pad)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ld_out = c.C + WIDER
    y = torch.empty(c.B * c.hw + GUARD, ld_out, device=DEV, dtype=torch.bfloat16)
    (out,) = twice(lambda: L().mkd_groupnorm(ptr(xb), c.C + c.pad, ptr(gd), ptr(bd), c.eps, silu, ptr(y), ld_out, c.B, c.hw, c.C, R.GROUPS, None),
                   [y], [xb, gd, bd])
    return inside(out, c.B * c.hw, c.C, f'{R.gn_id(c)} {name}').view(c.B, c.hw, c.C)


@pytest.mark.parametrize('c', R.GN_CASES, ids=[R.gn_id(c) for c in R.GN_CASES])
def test_groupnorm_elements(c):
    failures = []
    for name in c.sets:
        x, gamma, beta, ref, bnd = gn_host(name, c.B, c.hw, c.C, c.eps, c.silu)
        out = run_groupnorm(c, name, c.silu)
        line, fail = R.report(f'groupnorm {R.gn_id(c)} {name}', R.ratios(out, ref, bnd), lambda b, r, ch: R.locate(c.hw, c.C, b, r, ch))
        print(line)
        if fail:
            failures.append(fail)
        if name == 'degenerate':          # constant and all-zero groups: the bound is wide there (var = 0), but the kernel must not be
            cg = c.C // R.GROUPS
            for b in range(c.B):
                for gi in R.degenerate_groups(b):
                    err = (out[b, :, gi * cg:(gi + 1) * cg].double() - ref[b, :, gi * cg:(gi + 1) * cg]).abs().max()
                    print(f'NORMEL groupnorm {R.gn_id(c)} degenerate: sample {b} group {gi} largest |out - act(beta)| {err:.3e}')
    assert not failures, '; '.join(failures)


@pytest.mark.parametrize('C_,hw', R.FAR_GN)
def test_groupnorm_far_mean(C_, hw):
    """|mean| / std = 100: one-pass variance under cancellation.  Asserted: finite, and the a-priori bound (wide here by construction);
    measured and printed: per-group rel-L2 of the kernel and of torch's own group_norm on the same bf16 input (no SiLU: the same
    operation on both sides)."""
    c = next(c for c in R.GN_CASES if (c.C, c.hw) == (C_, hw))
    x, gamma, beta, ref, bnd = gn_host('far', c.B, c.hw, c.C, c.eps, 0)
    out = run_groupnorm(c, 'far', 0)
    line, fail = R.report(f'groupnorm {R.gn_id(c)} far', R.ratios(out, ref, bnd), lambda b, r, ch: R.locate(c.hw, c.C, b, r, ch))
    print(line)
    far_figures(f'groupnorm {R.gn_id(c)}', out, x, gamma, beta, c.eps, ref)
    assert fail is None, fail


def test_one_changed_pixel_shows_in_its_sample_alone():
    """The comparison itself, end to end on the device: the kernel is given the hard input with the last pixel of sample 0 replaced by the
    pixel before it, the reference keeps the original.  The statistics of every group of sample 0 move, so the OTHER pixels of every
    one of its groups leave the bound; sample 1 stays inside it."""
    c = next(c for c in R.GN_CASES if (c.C, c.hw) == (960, 1640))
    x, gamma, beta, ref, bnd = gn_host('hard', c.B, c.hw, c.C, c.eps, c.silu)
    xb = strided(x, c.C + c.pad)
    xb[c.hw - 1] = xb[c.hw - 2]
    y = torch.full((c.B * c.hw, c.C), NAN, device=DEV, dtype=torch.bfloat16)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rc = L().mkd_groupnorm(ptr(xb), c.C + c.pad, ptr(gd), ptr(bd), c.eps, c.silu, ptr(y), c.C, c.B, c.hw, c.C, R.GROUPS, None)
    assert rc == 0, L().mkd_last_error()
    sync()
    over = ~(R.ratios(y.cpu().float().view(c.B, c.hw, c.C), ref, bnd) <= 1.0)
    per_group = over[0, :-1].view(c.hw - 1, R.GROUPS, -1).sum((0, 2))
    print(f'NORMEL one changed pixel of {c.hw}: elements over the bound per group of sample 0: {per_group.min()} .. {per_group.max()} of {(c.hw - 1) * c.C // R.GROUPS}')
    assert (per_group > 0).all() and not over[1].any()


# ---- mkd_gn_colstats + mkd_gn_apply_stats ----------------------------------------------------------------------------------------------------
def colstats(c, xb, first_only=False):
    """The statistics of x in two column slices, as two producers of one tensor leave them."""
    ld, cg = c.C + c.pad, c.C // R.GROUPS
    gst = torch.zeros(c.B, R.GROUPS, 2, device=DEV, dtype=torch.int64)
    rc = L().mkd_gn_colstats(ptr(xb), ld, c.B, c.hw, c.split, cg, 0, ptr(gst), None)
    assert rc == 0, f'mkd_gn_colstats returned {rc}: {L().mkd_last_error()}'
    if not first_only:
        rc = L().mkd_gn_colstats(ptr(xb, 2 * c.split), ld, c.B, c.hw, c.C - c.split, cg, c.split, ptr(gst), None)
        assert rc == 0, f'mkd_gn_colstats returned {rc}: {L().mkd_last_error()}'
    sync()
    return gst


def run_split(c, name, silu):
    x, gamma, beta, ref, bnd = gn_host(name, c.B, c.hw, c.C, c.eps, silu)
    xb = strided(x, c.C + c.pad)
    keep = xb.clone()
    gst, again = colstats(c, xb), colstats(c, xb)
    assert torch.equal(gst, again), f'{name}: statistics not bit-repeatable'
    assert torch.equal(xb.view(torch.int16), keep.view(torch.int16)), 'mkd_gn_colstats changed its input'
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ld_out = c.C + WIDER
    y = torch.empty(c.B * c.hw + GUARD, ld_out, device=DEV, dtype=torch.bfloat16)
    (out,) = twice(lambda: L().mkd_gn_apply_stats(ptr(xb), c.C + c.pad, ptr(gd), ptr(bd), c.eps, silu, ptr(y), ld_out, c.B, c.hw, c.C, ptr(gst), None),
                   [y], [xb, gd, bd, gst])
    return inside(out, c.B * c.hw, c.C, f'split C{c.C}-hw{c.hw} {name}').view(c.B, c.hw, c.C), gst.cpu()


@pytest.mark.parametrize('c', R.STAT_CASES, ids=[f'C{c.C}-hw{c.hw}' for c in R.STAT_CASES])
def test_split_statistics_elements(c):
    failures = []
    cg = c.C // R.GROUPS
    for name in c.sets:
        silus = (0, 1) if name == 'degenerate' else (0,) if name == 'far' else (c.silu,)
        for silu in silus:
            x, gamma, beta, ref, bnd = gn_host(name, c.B, c.hw, c.C, c.eps, silu)
            out, gst = run_split(c, name, silu)
            tag = f'split C{c.C}-hw{c.hw} {name}' + (f' silu {silu}' if len(silus) > 1 else '')
            line, fail = R.report(tag, R.ratios(out, ref, bnd), lambda b, r, ch: R.locate_stat(c, b, r, ch))
            print(line)
            if fail:
                failures.append(fail)
            if name == 'far':
                far_figures(tag, out, x, gamma, beta, c.eps, ref)
            if name == 'degenerate':          # the all-zero group (q == 0: rstd = 1) gives exactly act(beta), rounded
                for b in range(c.B):
                    sl = slice(R.degenerate_groups(b)[0] * cg, (R.degenerate_groups(b)[0] + 1) * cg)
                    want = R.q16(ref[b, :, sl].float())
                    assert (gst[b, R.degenerate_groups(b)[0]] == 0).all()
                    if not torch.equal(out[b, :, sl], want):
                        failures.append(f'{tag}: the all-zero group {R.degenerate_groups(b)[0]} of sample {b} is not bf16(act(beta)): largest '
                                        f'difference {(out[b, :, sl] - want).abs().max():.3e}')
            if name == 'exact':               # small integers: the 64-bit fixed-point statistics are the integer sums, bit for bit
                xg = x.to(torch.int64).view(c.B, c.hw, R.GROUPS, cg)
                want = torch.stack([xg.sum((1, 3)) << 24, (xg * xg).sum((1, 3)) << 18], -1)
                if not torch.equal(gst, want):
                    b, g, k = (gst != want).nonzero()[0].tolist()
                    failures.append(f'{tag}: gstat[{b}][{g}][{k}] = {int(gst[b, g, k])}, the integer sum gives {int(want[b, g, k])}')
                first = colstats(c, strided(x, c.C + c.pad), first_only=True).cpu()
                touched = (c.split - 1) // cg + 1
                assert (first[:, touched:] == 0).all(), f'{tag}: the first slice wrote statistics of groups it does not cover'
                if c.split % cg == 0:
                    assert torch.equal(first[:, :touched], want[:, :touched])
    assert not failures, '; '.join(failures)


# ---- mkd_gemm_groupnorm_bf16 (gn_slab_kernel) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.SLAB_CASES, ids=[f'hw{c.H * c.W}' for c in R.SLAB_CASES])
def test_groupnorm_from_slabs_elements(c):
    """A split-K 3x3 conv whose output has hard per-group statistics -> gn_slab_kernel: the normalised output against the float64 GroupNorm
    of the raw tensor the same kernel stored, per element; and bit-equal to split-K reduce + mkd_groupnorm."""
    B, Cin, Cout, hw = R.SLAB_B, R.SLAB_CIN, R.SLAB_COUT, c.H * c.W
    M, K = B * hw, 9 * Cin
    x, w, bias, rowbias = R.slab_operands(c)
    gamma, beta = R.affine(Cout, 2)
    xb, wb = strided(x, Cin), strided(w, K)
    bd, rbd, gd, betad = bias.to(DEV), rowbias.to(DEV), gamma.to(DEV), beta.to(DEV)
    ld = Cout + WIDER
    raw = torch.empty(M + GUARD, ld, device=DEV, dtype=torch.bfloat16)
    y = torch.empty(M + GUARD, ld, device=DEV, dtype=torch.bfloat16)
    conv = (1, B, c.H, c.W, Cin, c.H, c.W, 1, 0)
    raw_c, y_c = twice(lambda: L().mkd_gemm_groupnorm_bf16(ptr(xb), Cin, ptr(wb), K, ptr(bd), ptr(rbd), Cout, hw, None, 0, 1.0, ptr(raw), ld, 1, M, Cout, K,
                                                           *conv, R.SLAB_SPLITK, hw, ptr(gd), ptr(betad), c.eps, c.silu, ptr(y), ld, None),
                       [raw, y], [xb, wb, bd, rbd, gd, betad])
    tag = f'slab hw{hw}'
    rawt = inside(raw_c, M, Cout, tag + ' raw').view(B, hw, Cout)
    out = inside(y_c, M, Cout, tag).view(B, hw, Cout)
    # the operands did make the statistics hard: standard deviations 1/4 .. 4, means up to several of them
    rg = rawt.double().view(B, hw, R.GROUPS, -1)
    sd, mu = rg.std((1, 3)), rg.mean((1, 3))
    assert sd.max() / sd.min() > 8 and (mu.abs() / sd).max() > 3
    ref, bnd = R.gn_ref(rawt, gamma, beta, c.eps, c.silu)
    line, fail = R.report(tag, R.ratios(out, ref, bnd), lambda b, r, ch: R.locate_slab(hw, Cout, b, r, ch))
    print(line)
    # the two-kernel path: split-K GEMM with its reduce kernel, then mkd_groupnorm
    raw2 = torch.full((M + GUARD, ld), NAN, device=DEV, dtype=torch.bfloat16)
    y2 = torch.full((M + GUARD, ld), NAN, device=DEV, dtype=torch.bfloat16)
    rc = L().mkd_gemm_bf16(ptr(xb), Cin, ptr(wb), K, ptr(bd), ptr(rbd), Cout, hw, None, 0, 1.0, 0, ptr(raw2), ld, 0, M, Cout, K, *conv, R.SLAB_SPLITK, None)
    assert rc == 0, L().mkd_last_error()
    rc = L().mkd_groupnorm(ptr(raw2), ld, ptr(gd), ptr(betad), c.eps, c.silu, ptr(y2), ld, B, hw, Cout, R.GROUPS, None)
    assert rc == 0, L().mkd_last_error()
    sync()
    assert torch.equal(raw2.cpu().view(torch.int16), raw_c.view(torch.int16)), 'raw output differs from the split-K reduce kernel'
    assert torch.equal(y2.cpu().view(torch.int16), y_c.view(torch.int16)), 'GroupNorm output differs from the two-kernel path'
    assert fail is None, fail


# ---- mkd_layernorm / mkd_layernorm_ld ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', R.LN_D)
@pytest.mark.parametrize('rows', R.LN_ROWS)
def test_layernorm_elements(rows, d):
    failures = []
    gamma, beta = R.affine(d, 1)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for name in R.LN_SETS:
        x = R.ln_input(name, rows, d)
        ref, bnd = R.ln_ref(x, gamma, beta, 1e-5)
        results = []
        for ldx in (0, d + 64, 5 * d):          # 0: mkd_layernorm (dense rows)
            xb = strided(x, ldx or d)
            y = torch.empty(rows + GUARD, d, device=DEV, dtype=torch.bfloat16)
            if ldx:
                launch = lambda: L().mkd_layernorm_ld(ptr(xb), ldx, ptr(gd), ptr(bd), 1e-5, ptr(y), rows, d, None)
            else:
                launch = lambda: L().mkd_layernorm(ptr(xb), ptr(gd), ptr(bd), 1e-5, ptr(y), rows, d, None)
            (out,) = twice(launch, [y], [xb, gd, bd])
            tag = f'layernorm {rows}x{d} ldx {ldx or d} {name}'
            out = inside(out, rows, d, tag)
            line, fail = R.report(tag, R.ratios(out, ref, bnd), lambda row, ch: R.locate_ln(d, row, ch))
            print(line)
            if fail:
                failures.append(fail)
            results.append(out)
        assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2]), f'{name}: the result depends on the input row stride'
    assert not failures, '; '.join(failures)


@pytest.mark.parametrize('d,want', sorted(R.LN_ERRORS.items()))
def test_layernorm_refuses_what_it_cannot_run(d, want):
    rows = 5
    x = torch.ones(rows, d + 8, device=DEV, dtype=torch.bfloat16)
    g = torch.ones(d + 8, device=DEV)
    y = torch.full((rows + GUARD, d + 8), NAN, device=DEV, dtype=torch.bfloat16)
    assert R.ln_branch_of(d) == want
    assert L().mkd_layernorm(ptr(x), ptr(g), ptr(g), 1e-5, ptr(y), rows, d, None) == want
    assert L().mkd_layernorm_ld(ptr(x), d + 8, ptr(g), ptr(g), 1e-5, ptr(y), rows, d, None) == want
    sync()
    assert torch.isnan(y.float()).all(), 'a refused call launched something'
