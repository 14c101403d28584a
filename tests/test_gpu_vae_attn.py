"""-m gpu: the first-stage mid-block attention as a stage (mkd_debug_vae_attn: the op sequence of mkd_ctx::vae_attn, with the
weights of a finalised decoder or encoder) against the float64 restatement of tests/vae_attn_ref.py, on scores that are hard for it:
q.weight and k.weight times 1, 2, 3 give logit std about 1, 4, 9.  Every output row is held to its own bound.

tests/test_vae_attn_ref_host.py shows on the same inputs that a pipeline with fp32 scores is inside these bounds and one with bf16
scores is outside them from logit std 4."""
import pytest
import torch

from gpu_util import DEV, L, P, assert_close_bf16, sync
import vae_attn_ref as R
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, VaeConfig

pytestmark = pytest.mark.gpu

UNET = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
            hint_widths=(16, 16, 32, 32, 32, 32, 64))
W_DEC, W_ENC = 2, 4
CASES = R.cases()
_engines = {}


def engine(net, which, s):
    """One context per (network, decoder / encoder, s), kept for the module: its weights are the seeded ones, q and k times s."""
    key = (net, which, s)
    if key not in _engines:
        ocfg = R.NETS[net]
        sd = R.scale_qk(R.state_dict(net, which), R.prefix(which), s)
        eng = MkdEngine(NetConfig(**UNET))
        vc = VaeConfig(z_channels=ocfg.z_channels, embed_dim=ocfg.embed_dim, ch=ocfg.ch, ch_mult=tuple(ocfg.ch_mult),
                       num_res_blocks=ocfg.num_res_blocks, out_ch=ocfg.out_ch)
        (eng.configure_vae if which == 'dec' else eng.configure_vae_encoder)(vc)
        for k, v in sd.items():
            eng.load_weight(k, v)
        (eng.finalize_vae if which == 'dec' else eng.finalize_vae_encoder)()
        _engines[key] = (eng, sd)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng, _ in _engines.values():
        eng.close()
    _engines.clear()


def run_stage(eng, which, x, want_o=True):
    B, H, W, C = x.shape
    xd = x.to(DEV).contiguous()
    out = torch.zeros_like(xd)
    o = torch.zeros(B * H * W, C, device=DEV, dtype=torch.bfloat16) if want_o else None
    rc = L().mkd_debug_vae_attn(eng._ctx, W_DEC if which == 'dec' else W_ENC, P(xd), B, H, W, C, P(out), P(o), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return o, out


@pytest.mark.parametrize('c', CASES, ids=[R.case_id(c) for c in CASES])
def test_stage_every_row(c):
    eng, sd = engine(c.net, c.which, c.s)
    x = R.make_x(c)
    o_ref, out_ref, info = R.stage(sd, R.prefix(c.which), x)
    o, out = run_stage(eng, c.which, x)
    o2, out2 = run_stage(eng, c.which, x)
    mo, mout = R.measures(o.cpu(), o_ref), R.measures(out.cpu(), out_ref)
    print(f'[vae_attn] {R.case_id(c)}: logit std {info["logit_std"]:.2f} max {info["logit_max"]:.1f}; '
          f'o whole {mo["whole"]:.2e} worst row {mo["row"]:.2e} max-abs {mo["maxabs"]:.2e}; '
          f'out whole {mout["whole"]:.2e} worst row {mout["row"]:.2e} max-abs {mout["maxabs"]:.2e}')
    for name, got, ref, m in (('o', o, o_ref, mo), ('out', out, out_ref, mout)):
        what = f'{R.case_id(c)} {name}'
        assert_close_bf16(got, ref, what=what)          # finite, rel-L2 <= 4e-3, max-abs <= 2^-6 |ref|_inf
        # Per row, no row left out: 8e-3 is twice the worst row (3.9e-3) of the fp32-score emulation on these inputs; the margin is
        # for MFMA accumulation order.  Measured on the MI355X, worst row over o and out, at s = 1 / 2 / 3:
        #   small dec 2x16x16  2.5e-3 / 3.6e-3 / 3.7e-3     small enc 2x16x16  2.4e-3 / 4.4e-3 / 3.6e-3
        #   small dec 3x4x12   2.7e-3 / 3.5e-3 / 3.5e-3     small enc 3x4x12   2.9e-3 / 3.6e-3 / 3.1e-3
        #   small dec 1x32x32  2.4e-3 / 3.8e-3 / 3.8e-3     small enc 1x32x32  2.6e-3 / 3.6e-3 / 3.9e-3
        #   real dec 1x8x8     2.0e-3 / 3.1e-3 / 2.9e-3     real dec 2x16x16   2.0e-3 / 4.9e-3 / 7.0e-3      spiked 3.7e-3
        # (whole rel-L2 1.7e-3 .. 2.3e-3 everywhere).  All but small enc 2x16x16 at s = 2 and real dec 2x16x16 equal the emulation to
        # two digits.  Supposed cause there, not isolated on the device: at real dec 2x16x16 an fp32 accumulation of the q|k GEMM
        # rounds about 70 of 524288 q|k elements to the other bf16 neighbour than float64 does (counted on the CPU); one such
        # element of magnitude 8..16 moves a logit by up to 0.03, and a row whose two largest weights are near 0.5 turns that into
        # 1e-2 of o.  Drawing 70 such elements at random on the CPU gave worst rows of 3.2e-3 .. 5.6e-3 in 30 draws.
        # With bf16 scores the same entry gave 1.5e-2 .. 9.3e-2 at s >= 2 (and 2.2e-3 .. 7.0e-3 at s = 1).
        assert m['row'] <= R.REL_ROW, f'{what}: worst row rel-L2 {m["row"]:.3e} > {R.REL_ROW:.1e}'
    assert torch.equal(o, o2) and torch.equal(out, out2), f'{R.case_id(c)}: two runs differ'


def test_o_may_be_null_and_the_decoder_plan_keeps_its_bits():
    """The entry's plan and workspace are its own: a decode (and an encode) after it gives the bits it gave before, at a shape whose
    attention (T = 64) is smaller than the stage's (T = 1024), and out does not depend on whether o is asked for."""
    c = R.Case('small', 'dec', 1, 32, 32, 2, False)
    eng, sd = engine(c.net, c.which, c.s)
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1)) * 0.18215
    d1 = eng.decode(z).cpu()
    x = R.make_x(c)
    _, out = run_stage(eng, 'dec', x)
    o_none, out_none = run_stage(eng, 'dec', x, want_o=False)
    assert o_none is None and torch.equal(out, out_none)
    assert torch.equal(eng.decode(z).cpu(), d1)
    enc, _ = engine('small', 'enc', 2)
    img = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(2)) * 2 - 1
    z1 = enc.encode(img).cpu()
    run_stage(enc, 'enc', R.make_x(R.Case('small', 'enc', 2, 16, 16, 2, False)))
    assert torch.equal(enc.encode(img).cpu(), z1)


def test_errors():
    lib = L()
    eng, _ = engine('small', 'dec', 1)
    x = torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.bfloat16)
    y = torch.zeros_like(x)
    assert lib.mkd_debug_vae_attn(eng._ctx, W_ENC, P(x), 1, 4, 4, 64, P(y), None, None) == -3          # no encoder in this context
    assert lib.mkd_debug_vae_attn(eng._ctx, W_DEC, None, 1, 4, 4, 64, P(y), None, None) == -1
    assert lib.mkd_debug_vae_attn(eng._ctx, W_DEC, P(x), 1, 4, 4, 64, None, None, None) == -1
    assert lib.mkd_debug_vae_attn(eng._ctx, W_DEC, P(x), 1, 4, 4, 32, P(y), None, None) == -1          # C != mid width
    assert lib.mkd_debug_vae_attn(eng._ctx, 3, P(x), 1, 4, 4, 64, P(y), None, None) == -1
    assert lib.mkd_debug_vae_attn(None, W_DEC, P(x), 1, 4, 4, 64, P(y), None, None) == -1
    plain = MkdEngine(NetConfig(**UNET))
    plain.configure_vae(VaeConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1))
    assert lib.mkd_debug_vae_attn(plain._ctx, W_DEC, P(x), 1, 4, 4, 64, P(y), None, None) == -3        # configured, not finalised
    plain.close()
