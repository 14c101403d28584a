"""No GPU: the float64 restatement of tests/vae_attn_ref.py agrees with oracle.vae._attn when its rounding is off, and the bounds
of tests/test_gpu_vae_attn.py tell the two orders of rounding apart on every input that test uses: a torch emulation of the intended
pipeline (fp32 scores, bf16 probabilities, bf16 o) is inside them on every case, the same with the scores rounded to bf16 is outside
them on every case with logit std >= 4 (q.weight and k.weight times 2 or 3)."""
import pytest
import torch

from oracle import vae
from tests import vae_attn_ref as R

CASES = R.cases()
IDS = [R.case_id(c) for c in CASES]
_cache = {}


def reference(c):
    if c not in _cache:
        p = R.prefix(c.which)
        sd = R.scale_qk(R.state_dict(c.net, c.which), p, c.s)
        x = R.make_x(c)
        _cache[c] = (sd, p, x) + R.stage(sd, p, x)
    return _cache[c]


def test_cases_are_the_ones_the_gpu_test_names():
    assert len(set(IDS)) == len(IDS) == 25
    assert {(c.net, c.which) for c in CASES} == {('small', 'dec'), ('small', 'enc'), ('real', 'dec')}
    assert R.width('small') == 64 and R.width('real') == 512
    assert {c.H * c.W for c in CASES if c.net == 'small'} == {256, 48, 1024} and {c.H * c.W for c in CASES if c.net == 'real'} == {64, 256}
    assert sum(c.spike for c in CASES) == 1


@pytest.mark.parametrize('which', ['dec', 'enc'])
def test_restatement_without_rounding_is_the_oracle(which):
    p = R.prefix(which)
    sd = R.scale_qk(R.state_dict('small', which), p, 2)
    x = torch.randn(2, 6, 8, 64, generator=torch.Generator().manual_seed(3))          # fp32 NHWC
    o, out, _ = R.stage(sd, p, x, rounding=False)
    want = vae._attn(sd, p, x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert (out.float() - want).abs().max() <= 1e-5 * max(1.0, want.abs().max().item())
    # o: what proj_out is applied to
    c = 64
    back = (out.double() - x.double() - sd[f'{p}.proj_out.bias'].double()).reshape(-1, c)
    assert (o @ sd[f'{p}.proj_out.weight'].reshape(c, c).double().T - back).abs().max() <= 1e-9


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_bounds_pass_fp32_scores_and_fail_bf16_scores(c):
    sd, p, x, o, out, info = reference(c)
    assert abs(info['logit_std'] / c.s ** 2 - 1.0) <= 0.2, info
    eo, eout = R.emulate(sd, p, x, 'fp32')
    mo, mout = R.measures(eo, o), R.measures(eout, out)
    print(f'{R.case_id(c)}: logit std {info["logit_std"]:.2f} max {info["logit_max"]:.1f}; fp32 scores: o {mo}, out {mout}')
    assert R.inside(mo) and R.inside(mout)
    # half the per-row bound: the margin the GPU test leaves for accumulation order
    assert mo['row'] <= R.REL_ROW / 2 and mout['row'] <= R.REL_ROW / 2
    bo, bout = R.emulate(sd, p, x, 'bf16')
    mo, mout = R.measures(bo, o), R.measures(bout, out)
    print(f'{R.case_id(c)}: bf16 scores: o {mo}, out {mout}')
    if c.s >= 2:
        assert mo['whole'] > R.REL_WHOLE and mo['row'] > R.REL_ROW, mo
        assert not R.inside(mout) and mout['row'] > R.REL_ROW, mout
