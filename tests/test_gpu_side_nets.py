"""-m gpu: the three side networks of a context (first-stage decoder, first-stage encoder, CLIP text encoder) share one life
cycle: a reloaded checkpoint takes effect at an unchanged shape and frees the fused weights of the previous one, and the plans
of the three nets, which share the auxiliary split-K / GroupNorm workspaces, do not disturb each other."""
import pytest
import torch

import vae_encoder_ref as enc_ref
from makeupdiffuse_amd.engine import ClipConfig, MkdEngine, NetConfig, VaeConfig
from oracle import clip as oc
from oracle import vae

pytestmark = pytest.mark.gpu

# the small configurations of tests/test_gpu_engine.py
SMALL = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
             hint_widths=(16, 16, 32, 32, 32, 32, 64))
VSMALL = dict(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2), num_res_blocks=1, out_ch=3)

VCFG = vae.VaeConfig(**VSMALL)                     # = make_encoder's ch=32, ch_mult=(1, 2), num_res_blocks=1
GEN = lambda seed: torch.Generator().manual_seed(seed)      # noqa: E731

# per net: configure the engine, the state dict of a seed, one call at the fixed input -> CPU tensor
NETS = {
    'decoder': (lambda e: e.configure_vae(VaeConfig(**VSMALL)),
                lambda seed: vae.init_state_dict(VCFG, seed=seed),
                lambda e, x: e.decode(x).cpu(),
                lambda: torch.randn(2, 4, 8, 8, generator=GEN(1)) * 0.18215),
    'encoder': (lambda e: e.configure_vae_encoder(VaeConfig(**VSMALL)),
                lambda seed: enc_ref.init_state_dict(VCFG, seed=seed),
                lambda e, x: torch.cat(e.encode(x, 0.18215, None, moments=True), dim=1).cpu(),       # z | moments
                lambda: torch.rand(2, 3, 64, 96, generator=GEN(2)) * 2 - 1),
    'clip': (lambda e: e.configure_clip(ClipConfig(**oc.SMALL.__dict__)),
             lambda seed: oc.init_state_dict(oc.SMALL, seed),
             lambda e, x: e.encode_tokens(x).cpu(),
             lambda: torch.randint(0, oc.SMALL.vocab_size, (2, 77), generator=GEN(3))),
}


def _load(eng, sd):
    for k, v in sd.items():
        eng.load_weight(k, v)


@pytest.mark.parametrize('kind', ['decoder', 'encoder', 'clip'])
def test_a_reloaded_side_net_takes_effect_and_does_not_grow_the_context(kind):
    """Every weight of the net loaded again, same shapes, same input shape: the output is that of an engine which only ever saw
    the new weights (the plan must not keep the previous checkpoint's fused block), and device_bytes() stays where it was (the
    previous fused block is freed).  Back to the first weights: the first output, bit for bit."""
    configure, state, run, make_input = NETS[kind]
    x = make_input()
    sd_a, sd_b = state(11), state(12)
    eng = MkdEngine(NetConfig(**SMALL))
    configure(eng)
    _load(eng, sd_a)
    out_a = run(eng, x)
    bytes_a = eng.device_bytes()
    fresh = MkdEngine(NetConfig(**SMALL))
    configure(fresh)
    _load(fresh, sd_b)
    ref_b = run(fresh, x)
    fresh.close()
    _load(eng, sd_b)
    out_b = run(eng, x)
    print(f'{kind}: bytes {bytes_a} -> {eng.device_bytes()}, equals fresh B {torch.equal(out_b, ref_b)}, equals A {torch.equal(out_b, out_a)}')
    assert torch.isfinite(out_a).all() and torch.isfinite(ref_b).all()
    assert torch.equal(out_b, ref_b)
    assert not torch.equal(out_b, out_a)
    assert eng.device_bytes() == bytes_a, (bytes_a, eng.device_bytes())
    _load(eng, sd_a)
    assert torch.equal(run(eng, x), out_a)
    assert eng.device_bytes() == bytes_a, (bytes_a, eng.device_bytes())
    eng.close()


def test_side_plans_do_not_disturb_each_other():
    """One context, three nets, interleaved calls that make every arena and the shared auxiliary workspaces grow: a repeated call
    returns its first result bit for bit."""
    eng = MkdEngine(NetConfig(**SMALL))
    for kind in ('decoder', 'encoder', 'clip'):
        configure, state, _, _ = NETS[kind]
        configure(eng)
        _load(eng, state(21))
    dec, enc, txt = NETS['decoder'][2], NETS['encoder'][2], NETS['clip'][2]
    z1 = NETS['decoder'][3]()
    z2 = torch.randn(2, 4, 16, 16, generator=GEN(4)) * 0.18215
    img, tok = NETS['encoder'][3](), NETS['clip'][3]()
    d1 = dec(eng, z1)
    e1 = enc(eng, img)
    t1 = txt(eng, tok)
    d2 = dec(eng, z2)
    assert torch.equal(dec(eng, z1), d1)
    assert torch.equal(enc(eng, img), e1)
    assert torch.equal(txt(eng, tok), t1)
    assert torch.equal(dec(eng, z2), d2)
    for o in (d1, e1, t1, d2):
        assert torch.isfinite(o).all()
    eng.close()
