"""-m gpu: the stand-alone attention kernels (csrc/kernels_attn.hip) through mkd_attention / mkd_attention_causal, per query row and
head, on every path launch_attention picks in the default build (tests/attention_ref.py: cases(), branch_of()):
  G   generic streaming kernel, 64-key tiles, 4 waves          C   one 96-key tile, 16-deep MFMA tail for dh 8 / 16 / 40 / 80
  W0  long self-attention, 8 waves (Tq, Tk >= 1024)            W1  the same with the row sums on the matrix cores (from 2048 keys)
  D   dh 40 long self-attention by LDS-DMA, 128-key tiles      K   causal (streaming kernel, 4 and 8 waves)
Every case asserts, for every (row, head),  max_d |out - ref| <= 2^-7 A  (A = max_d sum_j p_j |v_jd|; derivation in attention_ref.py)
against a float64 CPU reference on the bf16-rounded inputs, on input sets that make one fault the whole error of some row (designated
keys, q = 0, ascending / descending maxima, padding that would win; tests/test_attention_ref_host.py shows what each catches).  The
reference of branch D takes the queries as the kernel documents them (AttnCfg::OFFS): q' = bf16(float(q) * scale log2 e).

Not reached, by construction of the default build: attention_kernel<40, 8, 128, 2> (the non-DMA form of the dh-40 long path, taken only
when the MKD_ATTN_DMA knob is 0 in the environment: this file sets no knob and starts no process) and the paired launch (grid.z = 2,
a second AttnIo: only the engine passes one; the C ABI has no argument for it).

What the pre-scaled queries of branch D cost against the exact reference, CPU only (exact minus emulated-query float64 reference, from
test_attention_ref_host.py::test_prescaling_gap_of_the_dh40_long_path; no kernel output enters), worst row / rel-L2:
  130 keys  randn 2.1e-3 A / 8.2e-4,  4 x randn 1.5e-2 A / 3.0e-3        1153 keys  8.0e-4 A / 3.2e-4,  9.9e-3 A / 3.3e-3
  2049 keys 4.5e-4 A / 2.5e-4,  9.9e-3 A / 3.3e-3          (all below the suite's 8e-3 rel-L2 budget)

Measured on MI355X, worst err / (2^-7 A) over the cases of a branch (median of the per-case medians in brackets):
  G   soft 0.50 (0.07), hard 0.53 (0.17), uniform 0.21 (0.03), padding_would_win 0.35 (0.04), ascending 0.47 (0.07), descending 0.20 (0.04),
      designated 0.17 (0.00)
  C   soft 0.33 (0.06), hard 0.56 (0.16), uniform 0.12 (0.03), padding_would_win 0.23 (0.04), designated 0.08 (0.00)
  W0  soft 0.27 (0.06), hard 0.52 (0.19), uniform 0.06 (0.02), padding_would_win 0.26 (0.04), ascending 0.47 (0.23), descending 0.28 (0.07),
      designated 0.25 (0.00)
  W1  soft 0.26 (0.08), hard 0.47 (0.19), uniform 0.03 (0.03), padding_would_win 0.13 (0.05), ascending 0.43 (0.25), descending 0.20 (0.09),
      designated 0.25 (0.00)
  D   soft 0.26 (0.06), hard 0.56 (0.18), uniform 0.06 (0.03), padding_would_win 0.24 (0.03), ascending 0.56 (0.08), descending 0.13 (0.04),
      designated 0.07 (0.00)
  K   soft 0.46 (0.08), hard 0.52 (0.17), uniform 0.39 (0.04), padding_would_win 0.43 (0.06), ascending 0.57 (0.07), descending 0.51 (0.06),
      designated 0.09 (0.00)
The worst anywhere is 0.57 (K, 1040 x 1040 keys, ascending); the CPU emulation of a correct kernel reaches 0.56."""
import ctypes as C

import pytest
import torch

from tests import attention_ref as R
from tests.gpu_util import DEV, L, assert_close_bf16, sync

pytestmark = pytest.mark.gpu

CASES = R.cases()
NAN = float('nan')
GUARD = 128


def padded(x, ld, guard=0):
    """x [rows, n] (bf16 values) in the first columns of a NaN-filled [rows + guard, ld] bf16 device buffer."""
    rows, n = x.shape
    buf = torch.full((rows + guard, ld), NAN, dtype=torch.bfloat16)
    buf[:rows, :n] = x.to(torch.bfloat16)
    return buf.to(DEV)


def run_attention(c, q, k, v, scale):
    """Q with ldq > d; K | V as views of one [rows, 2 d + 8] buffer (the model's layout) or as two tensors (c.separate); O with
    ldo > d.  Stride gaps and 128 guard rows behind K, V and O hold NaN.  Two runs: bit-repeatable, finite inside the columns, NaN
    everywhere else."""
    B, Tq, Tk, heads, dh = c.B, c.Tq, c.Tk, c.heads, c.dh
    d = heads * dh
    ldq, ldo = d + 8, d + 4
    qb = padded(q, ldq)
    if c.separate:
        kb, vb = padded(k, d + 8, GUARD), padded(v, d + 8, GUARD)
        kp, vp, ldk = kb.data_ptr(), vb.data_ptr(), d + 8
    else:
        kvb = padded(torch.cat([k, v], 1), 2 * d + 8, GUARD)
        kp, vp, ldk = kvb.data_ptr(), kvb.data_ptr() + 2 * d, 2 * d + 8
    o = torch.full((B * Tq + GUARD, ldo), NAN, device=DEV, dtype=torch.bfloat16)
    fn = L().mkd_attention_causal if c.causal else L().mkd_attention

    def once():
        o.fill_(NAN)
        rc = fn(C.c_void_p(qb.data_ptr()), ldq, C.c_void_p(kp), ldk, C.c_void_p(vp), ldk, C.c_void_p(o.data_ptr()), ldo,
                B, Tq, Tk, heads, dh, scale, None)
        assert rc == 0, L().mkd_last_error()
        sync()
        return o.cpu()

    first, second = once(), once()
    assert torch.equal(first.view(torch.int16), second.view(torch.int16)), 'not bit-repeatable'
    out = second[:B * Tq, :d].float()
    assert torch.isfinite(out).all(), 'non-finite output'
    assert torch.isnan(second[:B * Tq, d:].float()).all() and torch.isnan(second[B * Tq:].float()).all(), 'wrote outside its rows / columns'
    return out


@pytest.mark.parametrize('c', CASES, ids=[R.case_id(c) for c in CASES])
def test_attention_rows(c):
    failures = []
    for name in R.sets_of(c):
        q, k, v, scale = R.build(name, c)
        q, k, v = R.q16(q), R.q16(k), R.q16(v)
        out = run_attention(c, q, k, v, scale)
        want, A = R.ref(q, k, v, c.B, c.Tq, c.Tk, c.heads, c.dh, scale, c.causal, prescale=c.branch == 'D')
        r = R.ratios(out, want, A, c.heads, c.dh)
        i = int(r.argmax())
        row, head = divmod(i, c.heads)
        print(f'ATTN {c.branch} {name} {R.case_id(c)}: worst err / (2^-7 A) {r.max():.3f} (row {row}, head {head}), median {r.median():.3f}')
        if not (r <= 1.0).all():
            failures.append(f'{name}: {int((r > 1.0).sum())} (row, head) over 2^-7 A, worst {r.max():.2f} at row {row}, head {head}')
        if name == 'soft':          # the suite's global check, against the exact reference on every branch
            exact = want if c.branch != 'D' else R.ref(q, k, v, c.B, c.Tq, c.Tk, c.heads, c.dh, scale, c.causal)[0]
            assert_close_bf16(out, exact, rel=8e-3, what=f'attention {R.case_id(c)}')
    assert not failures, f'{R.case_id(c)}: ' + '; '.join(failures)


def test_attention_rejects_what_it_does_not_cover():
    """Non-zero and no launch: the output stays NaN."""
    B, Tq, Tk, heads = 1, 16, 16, 2
    for dh, ldq_extra, tk, want in ((24, 0, Tk, -4), (48, 0, Tk, -4), (40, 4, Tk, None), (40, 0, 0, None)):
        d = heads * dh
        x = torch.zeros(B * 16, d + 8, device=DEV, dtype=torch.bfloat16)
        o = torch.full((B * Tq, d), NAN, device=DEV, dtype=torch.bfloat16)
        for fn in (L().mkd_attention, L().mkd_attention_causal):
            rc = fn(C.c_void_p(x.data_ptr()), d + ldq_extra, C.c_void_p(x.data_ptr()), d, C.c_void_p(x.data_ptr()), d, C.c_void_p(o.data_ptr()), d,
                    B, Tq, tk, heads, dh, dh ** -0.5, None)
            sync()
            assert rc != 0 and (want is None or rc == want), f'dh {dh} ldq {d + ldq_extra} Tk {tk}: rc {rc}'
            assert torch.isnan(o.float()).all()
