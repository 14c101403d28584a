"""-m gpu: the whole eps evaluation / DDIM loop through the C ABI vs the CPU oracle and the committed
golden fixtures.  Tolerances are SURVEY.md §8c's: one eps eval rel-L2 <= 2e-2, cosine >= 0.9995;
multi-step latents cosine >= 0.99 (bf16 compute, fp32 oracle)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from oracle import nets, sampler

pytestmark = pytest.mark.gpu


def _grouped():
    from makeupdiffuse_amd import lib as _mlib
    try:
        return bool(_mlib.load().mkd_grouped_launches_available())
    except Exception:
        return False


GROUPED = _grouped()
NEED_GROUP = ('grouped (2-problem) launches are an experiment build since round 4: tools/build_variant.sh group -DMKD_PAIR_N=2, '
              'MKD_LIB_PATH=makeupdiffuse_amd/libmkd_group.so (the default build has single-entry argument tables: +1.9 %)')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SMALL = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
             hint_widths=(16, 16, 32, 32, 32, 32, 64))


def check_eps(out, ref, rel=2e-2, cos=0.9995, what=''):
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), f'{what}: non-finite'
    r = ((out - ref).norm() / ref.norm()).item()
    c = F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    assert r <= rel and c >= cos, f'{what}: rel-L2 {r:.4e} (<= {rel}), cos {c:.6f} (>= {cos})'
    return r, c


@pytest.fixture(scope='module')
def small():
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    assert set(eng.expected_params()) == set(sd), 'engine and oracle disagree on the state_dict key set'
    eng.load_state_dict(sd)
    return eng, sd, ocfg, {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}


def test_small_eps_vs_golden(small):
    eng, sd, ocfg, g = small
    eng.prepare(g['hint'], g['ctx'])
    out = eng.eps(g['x'], g['t'])
    check_eps(out, g['eps'], what='eps')
    # same call again (plan re-use, no state leak)
    out2 = eng.eps(g['x'], g['t'])
    assert torch.equal(out, out2)


def test_small_eps_control_variants(small):
    eng, sd, ocfg, g = small
    eng.prepare(g['hint'], g['ctx'], control_scales=[float(s) for s in g['scales']])
    check_eps(eng.eps(g['x'], g['t']), g['eps_scaled'], what='control_scales')
    eng.prepare(g['hint'], g['ctx'], only_mid_control=True)
    check_eps(eng.eps(g['x'], g['t']), g['eps_mid'], what='only_mid_control')
    eng.prepare(None, g['ctx'], latent_hw=(8, 8))
    check_eps(eng.eps(g['x'], g['t']), g['eps_noctl'], what='c_concat None')


def test_small_eps_vs_oracle_other_shape(small):
    """non-square latent, batch 3, per-sample timesteps: oracle evaluated live."""
    eng, sd, ocfg, _ = small
    gen = torch.Generator().manual_seed(99)
    B, h, w = 3, 4, 12
    x = torch.randn(B, 4, h, w, generator=gen); hint = torch.rand(B, 6, 8 * h, 8 * w, generator=gen)
    ctx = torch.randn(B, 77, ocfg.context_dim, generator=gen); t = torch.tensor([1, 500, 999])
    ref = sampler.apply_model(sd, ocfg, x, t, {'c_crossattn': [ctx], 'c_concat': [hint]})
    eng.prepare(hint, ctx)
    check_eps(eng.eps(x, t), ref, what='eps 3x4x12')


def test_per_sample_independence(small):
    """B=2 must equal two B=1 evaluations (every op on the path is per-sample)."""
    eng, sd, ocfg, g = small
    eng.prepare(g['hint'], g['ctx'])
    both = eng.eps(g['x'], g['t']).clone()
    for i in range(2):
        eng.prepare(g['hint'][i:i + 1], g['ctx'][i:i + 1])
        one = eng.eps(g['x'][i:i + 1], g['t'][i:i + 1])
        check_eps(one, both[i:i + 1], rel=5e-3, cos=0.9999, what=f'sample {i}')


def test_small_sample_loop(small):
    eng, sd, ocfg, g = small
    sch = sampler.Schedule().make_ddim(5)
    eng.prepare(g['hint'], g['ctx'])
    out = eng.sample(g['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    r, c = check_eps(out, g['x5'], rel=1.5e-2, cos=0.9999, what='5-step latent')
    print(f'[parity] 5-step latent: rel-L2 {r:.4e} cos {c:.6f}')
    # hipGraph replay of the same loop (one captured step, device-resident step counter) must not change the numbers
    outg = eng.sample(g['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas,
                      use_graph=True)
    assert torch.allclose(outg, out, rtol=1e-5, atol=1e-6), (outg - out).abs().max()
    outg2 = eng.sample(g['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas,
                       use_graph=True)          # cached graph, counter re-armed
    assert torch.equal(outg, outg2)
    # several steps per captured graph (MKD_GRAPH_STEPS, default 5) + single-step remainder (make_ddim(7) has 8 steps = 5 + 3, make_ddim(12) 13 = 5 + 5 + 3, 4 = remainder only)
    for n in (7, 12, 4):
        s_n = sampler.Schedule().make_ddim(n)
        a_n = (s_n.ddim_timesteps, s_n.ddim_alphas, s_n.ddim_alphas_prev, s_n.ddim_sqrt_one_minus_alphas)
        assert torch.equal(eng.sample(g['x'], *a_n, use_graph=True), eng.sample(g['x'], *a_n, use_graph=False)), f'{n} steps: graph != eager'
    # CFG 9: prepared with 2B, unconditional first (cddim.py:25-31), hint shared (diffusion_makeup.py:401)
    eng.prepare(torch.cat([g['hint'], g['hint']]), torch.cat([g['uctx'], g['ctx']]))
    out = eng.sample(g['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas,
                     cfg_scale=9.0)
    r, c = check_eps(out, g['x5_cfg'], rel=6e-2, cos=0.999, what='5-step CFG latent')      # measured ~2.4e-2 (4-step CFG 9, round 2)
    print(f'[parity] 5-step CFG-9 latent: rel-L2 {r:.4e} cos {c:.6f}')
    outg = eng.sample(g['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas,
                      cfg_scale=9.0, use_graph=True)
    assert torch.allclose(outg, out, rtol=1e-5, atol=1e-6), (outg - out).abs().max()


def test_makeup_interpolation_vs_oracle(small):
    """BASELINE config 5 (build-defined: blend of the two cached hint embeddings): eps and a 5-step latent vs
    the oracle's restatement of the same definition; alpha = 0 / 1 must reduce to the single-reference path."""
    eng, sd, ocfg, g = small
    gen = torch.Generator().manual_seed(17)
    B = 3
    x = torch.randn(B, 4, 8, 8, generator=gen)
    src = torch.rand(B, 3, 64, 64, generator=gen); r1 = torch.rand(B, 3, 64, 64, generator=gen); r2 = torch.rand(B, 3, 64, 64, generator=gen)
    ctx = torch.randn(B, 77, ocfg.context_dim, generator=gen)
    h1, h2 = torch.cat([src, r1], 1), torch.cat([src, r2], 1)
    alpha = torch.tensor([0.0, 0.3, 1.0])
    t = torch.tensor([601, 601, 601])
    cond = {'c_crossattn': [ctx], 'c_concat': [h1], 'c_concat2': [h2], 'interp_alpha': alpha}
    ref = sampler.apply_model(sd, ocfg, x, t, cond)
    eng.prepare(h1, ctx, hint2=h2, alpha=alpha)
    out = eng.eps(x, t)
    check_eps(out, ref, what='interp eps')
    eng.prepare(h1, ctx)
    only1 = eng.eps(x, t)
    eng.prepare(h2, ctx)
    only2 = eng.eps(x, t)
    check_eps(out[0:1], only1[0:1], rel=1e-6, cos=0.999999, what='alpha=0 == reference 1')
    check_eps(out[2:3], only2[2:3], rel=1e-6, cos=0.999999, what='alpha=1 == reference 2')
    assert (out[1] - only1[1]).abs().max() > 1e-3 and (out[1] - only2[1]).abs().max() > 1e-3
    sch = sampler.Schedule().make_ddim(5)
    ref5 = sampler.sample(sampler.make_eps_fn(sd, ocfg), sampler.Schedule(), x, cond, 5)
    eng.prepare(h1, ctx, hint2=h2, alpha=alpha)
    out5 = eng.sample(x, sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas, use_graph=True)
    check_eps(out5, ref5, rel=6e-2, cos=0.99, what='interp 5-step latent')


VSMALL = dict(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2), num_res_blocks=1, out_ch=3)


def test_vae_decode_small_vs_oracle():
    from makeupdiffuse_amd.engine import VaeConfig
    from oracle import vae
    ocfg = vae.VaeConfig(**VSMALL)
    sd = vae.init_state_dict(ocfg, seed=5)
    eng = MkdEngine(NetConfig(**SMALL))
    eng.configure_vae(VaeConfig(**VSMALL))
    exp = {k for k in eng.expected_params() if k.startswith('first_stage_model.')}
    assert exp == set(sd), exp ^ set(sd)
    for k, v in sd.items():
        eng.load_weight(k, v)
    eng.finalize_vae()
    gen = torch.Generator().manual_seed(2)
    for (B, h, w) in [(2, 8, 8), (3, 4, 12)]:
        z = torch.randn(B, 4, h, w, generator=gen) * 0.18215
        ref = vae.decode_first_stage(sd, ocfg, z)
        out = eng.decode(z)
        assert out.shape == ref.shape == (B, 3, 2 * h, 2 * w)
        check_eps(out, ref, rel=1.5e-2, cos=0.9997, what=f'vae decode {B}x{h}x{w}')
    eng.close()


@pytest.mark.timeout(600)
def test_vae_decode_full_size_vs_oracle():
    """SD-1.x decoder of the yaml (49.49 M params), one 32x32 latent -> 256x256 image, vs the fp32 CPU oracle."""
    from makeupdiffuse_amd.engine import VaeConfig
    from oracle import vae
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    sd = vae.init_state_dict(vae.FULL, seed=0)
    eng = MkdEngine(NetConfig(**SMALL))
    eng.configure_vae(VaeConfig())
    for k, v in sd.items():
        eng.load_weight(k, v)
    eng.finalize_vae()
    z = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(3)) * 0.18215
    ref = vae.decode_first_stage(sd, vae.FULL, z)
    out = eng.decode(z)
    r, c = check_eps(out, ref, rel=2e-2, cos=0.9995, what='full-size vae decode')
    print(f'full-size vae decode: rel-L2 {r:.4e} cos {c:.6f} GFLOP {eng.decode_flops() / 1e9:.1f}')
    eng.close()


def test_param_counts_full():
    eng = MkdEngine(NetConfig())
    assert abs(eng.param_count('unet') / 1e6 - 859.52) < 0.01
    assert abs(eng.param_count('control') / 1e6 - 361.28) < 0.01
    eng.close()


def test_missing_weight_is_loud():
    from makeupdiffuse_amd.lib import MkdError
    eng = MkdEngine(NetConfig(**SMALL))
    with pytest.raises(MkdError):
        eng.finalize()
    with pytest.raises(MkdError):
        eng.prepare(torch.rand(1, 6, 64, 64), torch.randn(1, 77, 64))


@pytest.mark.timeout(900)
def test_full_size_eps_vs_oracle():
    """BASELINE full architecture (859.5 M + 361.3 M params), B=1, 256x256: one eps eval vs the fp32 CPU oracle."""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    cfg = nets.FULL
    sd = nets.init_state_dict(cfg, seed=0)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, 32, 32, generator=gen); hint = torch.rand(1, 6, 256, 256, generator=gen)
    ctx = torch.randn(1, 77, 768, generator=gen); t = torch.tensor([501])
    ref = sampler.apply_model(sd, cfg, x, t, {'c_crossattn': [ctx], 'c_concat': [hint]})
    eng = MkdEngine(NetConfig())
    eng.load_state_dict(sd)
    sd_ref = sd
    del sd
    eng.prepare(hint, ctx)
    r, c = check_eps(eng.eps(x, t), ref, what='full-size eps')
    print(f'full-size eps: rel-L2 {r:.4e} cos {c:.6f} launches {eng.eps_launches()} GFLOP {eng.eps_flops() / 1e9:.1f}')
    # the same evaluation with the fused transformer tail forced on (batch 1 is below its shape policy's threshold)
    os.environ['MKD_TFM_TAIL'] = '1'
    try:
        eng_f = MkdEngine(NetConfig())
    finally:
        os.environ.pop('MKD_TFM_TAIL')
    eng_f.load_state_dict(sd_ref)
    eng_f.prepare(hint, ctx)
    rf, cf = check_eps(eng_f.eps(x, t), ref, what='full-size eps, fused transformer tail')
    print(f'full-size eps, fused transformer tail: rel-L2 {rf:.4e} cos {cf:.6f} launches {eng_f.eps_launches()}')
    # (7 d = 320 blocks; at batch 1 the unfused tail is 6 launches - LayerNorm 3 is taken on the fly there - against 1, and the
    # unfused head 3 - GroupNorm, proj_in, q|k|v with LayerNorm 1 on the fly - against statistics + head)
    assert eng.eps_launches() - eng_f.eps_launches() == 42 and abs(eng_f.eps_flops() - eng.eps_flops()) < 1e6
    eng_f.close()
    # 121.42 GMAC per sample per eval, minus what mkd_prepare caches once per batch:
    # hint block 1.87 GMAC + cross-attention K/V projections 2.16 GMAC -> 117.39 GMAC executed per eval
    assert abs(eng.eps_flops() / 2e9 - 117.39) < 0.05
    # BASELINE config 5 at full size: the blended hint embedding (alpha = 0.4 between two references) vs the oracle's restatement
    hint2 = torch.cat([hint[:, :3], torch.rand(1, 3, 256, 256, generator=gen)], 1)
    alpha = torch.tensor([0.4])
    ref_i = sampler.apply_model(sd_ref, cfg, x, t, {'c_crossattn': [ctx], 'c_concat': [hint], 'c_concat2': [hint2], 'interp_alpha': alpha})
    eng.prepare(hint, ctx, hint2=hint2, alpha=alpha)
    out_i = eng.eps(x, t)
    r, c = check_eps(out_i, ref_i, what='full-size interpolation eps')
    print(f'full-size interpolation eps (alpha 0.4): rel-L2 {r:.4e} cos {c:.6f}')
    assert (ref_i - ref).abs().max() > 1e-3          # the second reference does change the result
    # the remaining apply_model variants at full size (makeup_diffuse.py:164-170): decaying control_scales, only_mid_control, no hint
    cond = {'c_crossattn': [ctx], 'c_concat': [hint]}
    scales = [0.825 ** (12 - i) for i in range(13)]
    for what, okw, ekw in (('control_scales', dict(control_scales=scales), dict(control_scales=scales)),
                           ('only_mid_control', dict(only_mid_control=True), dict(only_mid_control=True))):
        ref_v = sampler.apply_model(sd_ref, cfg, x, t, cond, **okw)
        eng.prepare(hint, ctx, **ekw)
        r, c = check_eps(eng.eps(x, t), ref_v, what=f'full-size eps, {what}')
        print(f'full-size eps, {what}: rel-L2 {r:.4e} cos {c:.6f}')
        assert (ref_v - ref).abs().max() > 1e-3
    ref_n = sampler.apply_model(sd_ref, cfg, x, t, {'c_crossattn': [ctx], 'c_concat': None})
    eng.prepare(None, ctx, latent_hw=(32, 32))
    r, c = check_eps(eng.eps(x, t), ref_n, what='full-size eps, c_concat None')
    print(f'full-size eps, c_concat None: rel-L2 {r:.4e} cos {c:.6f}')
    eng.close()


@pytest.mark.parametrize('dec_lanes,enc_lanes,overlap,helpers,group',
                         [(0, 0, 1, 0, 0), (0, 0, 0, 0, 0), (2, 0, 1, 0, 0), (2, 0, 1, 1, 0), (4, 0, 1, 0, 0), (2, 1, 1, 1, 0), (4, 1, 1, 0, 0),
                          (0, 0, 1, 0, 1), (0, 0, 0, 0, 1), (2, 0, 1, 0, 1), (2, 0, 1, 1, 1), (4, 0, 1, 0, 1)])
def test_stream_lanes_are_race_free_and_match_golden(dec_lanes, enc_lanes, overlap, helpers, group, monkeypatch):
    """Every multi-stream configuration (decoder helpers on the side stream, half-/quarter-batch decoder lanes, half-batch
    encoder lanes; the encoder phase as two chains on two streams or as one chain of grouped launches): NaN-poison all buffers an
    evaluation produces, evaluate, and require the golden result, bit-identical
    across repetitions - a kernel that runs ahead of its producer would read NaN instead of the previous call's values."""
    monkeypatch.setenv('MKD_DEC_LANES', str(dec_lanes)); monkeypatch.setenv('MKD_ENC_LANES', str(enc_lanes))
    if group and not GROUPED:
        pytest.skip(NEED_GROUP)
    monkeypatch.setenv('MKD_DEC_OVERLAP', str(overlap)); monkeypatch.setenv('MKD_LANE_HELPERS', str(helpers))
    monkeypatch.setenv('MKD_ENC_GROUP', str(group))
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    eng.load_state_dict(sd)
    G = {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}
    rep = lambda t: torch.cat([t, t, t[:1]])                      # batch 5: ragged lanes (1+1+1+2 or 2+3)
    for hint, want in ((rep(G['hint']), rep(G['eps'])), (None, rep(G['eps_noctl']))):
        eng.prepare(hint, rep(G['ctx']), latent_hw=(8, 8))
        first = None
        for i in range(4):
            eng.debug_poison()
            out = eng.eps(rep(G['x']), rep(G['t']))
            check_eps(out, want, what=f'lanes dec={dec_lanes} enc={enc_lanes} overlap={overlap} group={group} rep {i}')
            first = out if first is None else first
            assert torch.equal(out, first)
        # the captured-graph loop takes the same plan
        sch_t = [801, 601, 401, 201]
        eng.debug_poison()
        a = eng.sample(rep(G['x']), sch_t, [0.1, 0.3, 0.6, 0.9], [0.3, 0.6, 0.9, 0.99], [0.95, 0.84, 0.63, 0.31], use_graph=False)
        eng.debug_poison()
        b = eng.sample(rep(G['x']), sch_t, [0.1, 0.3, 0.6, 0.9], [0.3, 0.6, 0.9, 0.99], [0.95, 0.84, 0.63, 0.31], use_graph=True)
        assert torch.isfinite(a).all() and torch.equal(a, b)
    eng.close()


@pytest.mark.parametrize('dec_lanes', [0, 2])
def test_groupnorm_producer_statistics_plan_matches_golden(dec_lanes, monkeypatch):
    """MKD_GN_FUSED=1: every GroupNorm reads statistics that the kernels writing its input accumulated (GEMM / LDS-staged conv /
    split-K epilogues, the copy fallback on the c_concat None path) and only applies them.  Same golden eps, bit-repeatable after
    NaN-poisoning (integer atomics are order-free), graph replay == eager launches."""
    monkeypatch.setenv('MKD_GN_FUSED', '1'); monkeypatch.setenv('MKD_DEC_LANES', str(dec_lanes))
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    eng.load_state_dict(sd)
    G = {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}
    rep = lambda t: torch.cat([t, t, t[:1]])
    for hint, want in ((rep(G['hint']), rep(G['eps'])), (None, rep(G['eps_noctl']))):
        eng.prepare(hint, rep(G['ctx']), latent_hw=(8, 8))
        first = None
        for i in range(3):
            eng.debug_poison()
            out = eng.eps(rep(G['x']), rep(G['t']))
            check_eps(out, want, what=f'fused GroupNorm statistics, lanes {dec_lanes}, rep {i}')
            first = out if first is None else first
            assert torch.equal(out, first)
    sch = sampler.Schedule().make_ddim(5)
    args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    eng.prepare(G['hint'], G['ctx'])
    a = eng.sample(G['x'], *args, use_graph=False)
    b = eng.sample(G['x'], *args, use_graph=True)
    check_eps(a, G['x5'], rel=1.5e-2, cos=0.9999, what='5-step latent, fused GroupNorm statistics')
    assert torch.equal(a, b)
    eng.close()


@pytest.mark.parametrize('mask', [0, 2, 7])
def test_layernorm_on_the_fly_plans_match_golden(mask, monkeypatch):
    """MKD_LN_FLY bit mask (norm1 / norm2 / norm3 folded into the consuming GEMM, row statistics taken inside it): every choice
    gives the golden eps (with the fixture's random LayerNorm gamma / beta), bit-repeatable after poisoning, graph == eager."""
    monkeypatch.setenv('MKD_LN_FLY', str(mask))
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    eng.load_state_dict(sd)
    G = {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}
    eng.prepare(G['hint'], G['ctx'])
    first = None
    for i in range(3):
        eng.debug_poison()
        out = eng.eps(G['x'], G['t'])
        check_eps(out, G['eps'], what=f'MKD_LN_FLY={mask} rep {i}')
        first = out if first is None else first
        assert torch.equal(out, first)
    sch = sampler.Schedule().make_ddim(5)
    args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    a = eng.sample(G['x'], *args, use_graph=False)
    b = eng.sample(G['x'], *args, use_graph=True)
    check_eps(a, G['x5'], rel=1.5e-2, cos=0.9999, what=f'5-step latent, MKD_LN_FLY={mask}')
    assert torch.equal(a, b)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('lanes', [0, 2])
def test_linear_graph_segments_equal_the_eager_loop(lanes, monkeypatch):
    """MKD_GRAPH_MODE=2: a step replayed as per-stream LINEAR graphs ordered by events (instead of one captured graph with branches)
    gives the eager loop's latents bit for bit - plain and with guidance, cached segments re-used, with and without decoder lanes."""
    monkeypatch.setenv('MKD_GRAPH_MODE', '2')
    monkeypatch.setenv('MKD_DEC_LANES', str(lanes))
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    eng.load_state_dict(sd)
    G = {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}
    sch = sampler.Schedule().make_ddim(5)
    args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    eng.prepare(G['hint'], G['ctx'])
    a = eng.sample(G['x'], *args, use_graph=False)
    b = eng.sample(G['x'], *args, use_graph=True)
    c = eng.sample(G['x'], *args, use_graph=True)          # cached segments
    check_eps(a, G['x5'], rel=1.5e-2, cos=0.9999, what='5-step latent, linear graph segments')
    assert torch.equal(a, b) and torch.equal(a, c)
    eng.prepare(torch.cat([G['hint'], G['hint']]), torch.cat([G['uctx'], G['ctx']]))
    d = eng.sample(G['x'], *args, cfg_scale=9.0, use_graph=False)
    e = eng.sample(G['x'], *args, cfg_scale=9.0, use_graph=True)
    assert torch.equal(d, e)
    eng.close()


def _small_engine():
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    ocfg = nets.NetConfig(**SMALL)
    sd = nets.init_state_dict(ocfg, seed=int(g['seed_weights']))
    eng = MkdEngine(NetConfig(**SMALL))
    eng.load_state_dict(sd)
    return eng, {k: torch.from_numpy(g[k]) for k in g.files if k not in ('seed_weights', 'seed_vae')}


@pytest.mark.parametrize('dec_lanes', [0, 2])
def test_grouped_encoder_equals_the_two_chain_plan_bit_for_bit(dec_lanes, monkeypatch):
    """MKD_ENC_GROUP: ControlNet and UNet encoder + middle block as ONE chain of grouped (2-problem) launches against two chains on
    two streams (reference diffmk/makeup_diffuse.py:164-168, the two net calls of apply_model).  Same kernels, same tiles, same
    order of operations per output element: the eps of a ragged batch, the 5-step latent (eager and graph replay) and the guided
    loop are equal BIT FOR BIT, after NaN-poisoning; the grouped plan has one launch per encoder op pair."""
    if not GROUPED:
        pytest.skip(NEED_GROUP)
    monkeypatch.setenv('MKD_DEC_LANES', str(dec_lanes))
    res = {}
    for group in (0, 1):
        monkeypatch.setenv('MKD_ENC_GROUP', str(group))
        eng, G = _small_engine()
        rep = lambda t: torch.cat([t, t, t[:1]])
        eng.prepare(rep(G['hint']), rep(G['ctx']))
        eng.debug_poison()
        e5 = eng.eps(rep(G['x']), rep(G['t']))
        check_eps(e5, rep(G['eps']), what=f'MKD_ENC_GROUP={group}')
        n_eps = eng.eps_launches()
        sch = sampler.Schedule().make_ddim(5)
        args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
        eng.prepare(G['hint'], G['ctx'])
        eng.debug_poison()
        a = eng.sample(G['x'], *args, use_graph=False)
        eng.debug_poison()
        b = eng.sample(G['x'], *args, use_graph=True)
        assert torch.equal(a, b)
        eng.prepare(torch.cat([G['hint'], G['hint']]), torch.cat([G['uctx'], G['ctx']]))
        c = eng.sample(G['x'], *args, cfg_scale=9.0, use_graph=True)
        eng.prepare(None, G['ctx'], latent_hw=(8, 8))            # c_concat None: nothing to group, same plan either way
        d = eng.eps(G['x'], G['t'])
        res[group] = (e5, a, c, d, n_eps)
        eng.close()
    for k in range(4):
        assert torch.equal(res[0][k], res[1][k]), f'grouped plan differs from the two-chain plan (output {k})'
    check_eps(res[1][1], G['x5'], rel=1.5e-2, cos=0.9999, what='5-step latent, grouped encoder')
    print(f'launches per eps: two chains {res[0][4]}, grouped {res[1][4]}')
    assert res[1][4] < res[0][4] - 20, 'the grouped plan must launch once per encoder op pair'


def test_time_embedding_table_equals_the_per_step_chain_bit_for_bit(monkeypatch):
    """mkd_sample computes the time embedding of ALL its steps once per call (timesteps are a host table, reference
    diffmk/cddim.py:83-95) and a step only copies its row; MKD_TEMB_TABLE=0 runs the chain of mkd_eps in every step.  Latents are
    equal bit for bit (eager, graph replay, guidance, a second call with other timesteps), and equal to stepping by hand with mkd_eps
    + mkd_ddim_step; a step inside the loop launches less than a stand-alone mkd_eps."""
    res = {}
    for table in (0, 1):
        monkeypatch.setenv('MKD_TEMB_TABLE', str(table))
        eng, G = _small_engine()
        sch = sampler.Schedule().make_ddim(5)
        args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
        eng.prepare(G['hint'], G['ctx'])
        a = eng.sample(G['x'], *args, use_graph=False)
        b = eng.sample(G['x'], *args, use_graph=True)
        sch7 = sampler.Schedule().make_ddim(7)
        args7 = (sch7.ddim_timesteps, sch7.ddim_alphas, sch7.ddim_alphas_prev, sch7.ddim_sqrt_one_minus_alphas)
        c = eng.sample(G['x'], *args7, use_graph=True)            # another step count: the table is re-built
        b2 = eng.sample(G['x'], *args, use_graph=True)
        e = eng.eps(G['x'], G['t'])                               # a stand-alone evaluation after a loop runs its own chain again
        check_eps(e, G['eps'], what=f'eps after a sampling loop, MKD_TEMB_TABLE={table}')
        # by hand: mkd_eps + mkd_ddim_step per step
        x = G['x'].to(eng.device)
        for i in range(4, -1, -1):
            t = torch.full((x.shape[0],), int(sch.ddim_timesteps[i]), dtype=torch.int64)
            ee = eng.eps(x, t)
            x, _ = eng.ddim_step(x, ee, None, 1.0, float(sch.ddim_alphas[i]), float(sch.ddim_alphas_prev[i]), 0.0,
                                 float(sch.ddim_sqrt_one_minus_alphas[i]))
        assert torch.equal(a, b) and torch.equal(b, b2) and torch.equal(a, x.to(a.device))
        eng.prepare(torch.cat([G['hint'], G['hint']]), torch.cat([G['uctx'], G['ctx']]))
        d = eng.sample(G['x'], *args, cfg_scale=9.0, use_graph=True)
        res[table] = (a, c, d, e, eng.step_launches(), eng.eps_launches())
        eng.close()
    for k in range(4):
        assert torch.equal(res[0][k], res[1][k]), f'table-fed loop differs from the per-step chain (output {k})'
    print(f'launches per step: chain {res[0][4]}, table {res[1][4]} (stand-alone eps {res[1][5]})')
    assert res[1][4] <= res[0][4] - 6


def test_split_setting_changed_after_prepare_is_loud_then_replanned(monkeypatch):
    """A split conv1 -> GroupNorm pair is planned for a fixed slab count (op_gemm_then_gn; MKD_GN_SLAB_MINC=64 turns it on for a
    256-channel test net).  Changing the split-K cap after mkd_prepare must not silently reduce the wrong number of slabs: the stale
    plan's launch fails loudly, and the next mkd_prepare re-plans (the plan epoch moved) and agrees with the first result."""
    from makeupdiffuse_amd import lib as mlib
    monkeypatch.setenv('MKD_GN_SLAB_MINC', '64')
    cfg = NetConfig(model_channels=256, channel_mult=(1,), attention_resolutions=(1,), num_heads=4, context_dim=64,
                    hint_widths=(16, 16, 32, 32, 32, 32, 64))
    eng = MkdEngine(cfg)
    eng.init_random(0, norm_jitter=0.2)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 8, 8, generator=g); hint = torch.rand(2, 6, 64, 64, generator=g); ctx = torch.randn(2, 77, 64, generator=g)
    t = torch.tensor([801, 41])
    eng.prepare(hint, ctx)
    ref = eng.eps(x, t)
    assert torch.isfinite(ref).all()
    try:
        monkeypatch.setenv('MKD_SPLITK_CAP', '1')                 # read by mkd_ctx_create: process-wide cap, no GEMM splits K any more
        other = MkdEngine(NetConfig(**SMALL))
        with pytest.raises(mlib.MkdError, match='prepare again'):
            eng.eps(x, t)
        torch.cuda.synchronize()
        eng.prepare(hint, ctx)                                    # re-planned: nothing is split, nothing deferred
        check_eps(eng.eps(x, t), ref, rel=1e-2, what='re-planned without split-K')
        other.close()
    finally:
        monkeypatch.setenv('MKD_SPLITK_CAP', '0')
        last = MkdEngine(NetConfig(**SMALL))                      # (lifts the cap again)
        last.close()
    eng.prepare(hint, ctx)
    assert torch.equal(eng.eps(x, t), ref)
    eng.close()


def test_xcd_auto_order_changes_no_bit(monkeypatch):
    """MKD_XCD_AUTO_RATIO: the weight-heavy GEMMs / convolutions (M <= ratio x N) walk their tiles in XCD-contiguous runs so that a weight
    tile is pulled through one L2; the workgroup -> tile map is a permutation, so eps and the 5-step latent are equal BIT FOR BIT to
    launch order everywhere (ratio 0) and to the remap everywhere (ratio 1e9)."""
    res = {}
    for ratio in ('0', '2', '1e9'):
        monkeypatch.setenv('MKD_XCD_AUTO_RATIO', ratio)
        eng, G = _small_engine()
        rep = lambda t: torch.cat([t, t, t[:1]])
        eng.prepare(rep(G['hint']), rep(G['ctx']))
        eng.debug_poison()
        e = eng.eps(rep(G['x']), rep(G['t']))
        sch = sampler.Schedule().make_ddim(5)
        eng.prepare(G['hint'], G['ctx'])
        lat = eng.sample(G['x'], sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas, use_graph=True)
        res[ratio] = (e, lat)
        eng.close()
    check_eps(res['2'][0], torch.cat([G['eps'], G['eps'], G['eps'][:1]]), what='default XCD order')
    for r in ('0', '1e9'):
        assert torch.equal(res[r][0], res['2'][0]) and torch.equal(res[r][1], res['2'][1]), f'MKD_XCD_AUTO_RATIO={r} changed the result'


def test_plan_options_are_per_context():
    """plan switches live in the context (mkd_ctx_set_option: the next prepare re-plans, another context is not
    touched).  The tile tuner's state stays process-global by design (include/mkd.h): a change re-plans every live context
    (test_split_setting_changed_after_prepare_is_loud_then_replanned)."""
    import ctypes as C
    from makeupdiffuse_amd import lib as mlib
    e1 = MkdEngine(NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                             hint_widths=(16, 16, 32, 32, 32, 32, 64)))
    e1.init_random(3, norm_jitter=0.2)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 4, 16, 16, generator=g); hint = torch.rand(4, 6, 128, 128, generator=g); ctx = torch.randn(4, 77, 64, generator=g)
    t = torch.tensor([901, 601, 301, 1])
    e1.prepare(hint, ctx)
    a = e1.eps(x, t); n2 = e1.eps_launches()
    assert e1.get_option('dec_lanes') == 2 and e1.get_option('gn_2k_min_hw') == 4096 and e1.get_option('xcd_auto_ratio') == 1
    e1.set_option('dec_lanes', 0)
    e1.prepare(hint, ctx)                                   # same arguments: re-plans because an option changed
    b = e1.eps(x, t)
    # no lanes: fewer launches; the full-batch decoder takes other tiles / split-K than the half-batch lanes: same values within the bf16 budget
    assert e1.eps_launches() < n2 and float((b.float() - a.float()).norm() / a.float().norm()) < 1e-2
    e1.set_option('gn_2k_min_hw', 64)                       # every GroupNorm with >= 64 pixels as two full-chip launches
    e1.prepare(hint, ctx)
    c = e1.eps(x, t)
    assert float((c.float() - a.float()).norm() / a.float().norm()) < 2e-2      # (another plan of the same bf16 nets: measured 1.1e-2)
    with pytest.raises(mlib.MkdError):
        e1.set_option('no_such_option', 1)
    lib = mlib.load()
    n_live = lib.mkd_live_contexts()
    e2 = MkdEngine(NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                             hint_widths=(16, 16, 32, 32, 32, 32, 64)))
    try:
        assert lib.mkd_live_contexts() == n_live + 1
        assert e2.get_option('dec_lanes') == 2              # the other context's option did not leak
    finally:
        e2.close()
    assert lib.mkd_live_contexts() == n_live
    e1.close()


def test_reloading_weights_frees_the_derived_copies_and_invalidates_the_plan():
    """finalize() derives weight forms (q|k|v and K|V concatenations, LayerNorm folds, merged FF2 . proj_out, packed transformer
    streams, [W_conv2 | W_skip]): a second load of the weights rebuilds them and frees the previous generation - device memory does not
    grow - and the prepared plan of the old weights is refused until mkd_prepare ran again."""
    from makeupdiffuse_amd import lib as mlib
    e = MkdEngine(NetConfig(**SMALL))
    e.init_random(3, norm_jitter=0.2)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 16, generator=g); hint = torch.rand(2, 6, 128, 128, generator=g); ctx = torch.randn(2, 77, 64, generator=g)
    t = torch.tensor([801, 201])
    e.prepare(hint, ctx)
    a = e.eps(x, t); b0 = e.device_bytes()
    e.init_random(3, norm_jitter=0.2)                   # every weight again: finalized -> false, plan invalid
    with pytest.raises(mlib.MkdError):
        e.eps(x, t)
    e.prepare(hint, ctx)
    b = e.eps(x, t)
    assert torch.equal(a, b)
    assert e.device_bytes() <= b0 + (1 << 20), (b0, e.device_bytes())
    e.init_random(4, norm_jitter=0.2)
    e.prepare(hint, ctx)
    assert not torch.equal(e.eps(x, t), a) and e.device_bytes() <= b0 + (1 << 20)
    e.close()


# ---- the exported entry each option combination reaches (MkdEngine._sample_call / _step_call) ------------------------------------------
class _Recorder:
    """eng.lib behind a proxy that notes every mkd_sample* / mkd_<solver>_step* symbol called through it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith('mkd_sample') or name.split('_step')[0] in ('mkd_ddim', 'mkd_dpmpp', 'mkd_unipc')):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


@pytest.fixture(scope='module')
def recorded():
    eng, g = _small_engine()
    rec = _Recorder(eng.lib)
    eng.lib = rec
    yield eng, g, rec
    eng.lib = rec._lib
    eng.close()


# (method, trace, guidance rescale, masked, eta) -> the entry; the rows of the table in MkdEngine._sample_call's docstring
LOOP_ENTRIES = [
    ('sample', True, 0.0, False, False, 'mkd_sample_masked_ex'),
    ('sample', False, 0.7, True, True, 'mkd_sample_masked_ex'),
    ('sample', True, 0.7, True, False, 'mkd_sample_masked_ex'),
    ('sample', False, 0.0, True, False, 'mkd_sample_masked'),
    ('sample', False, 0.0, True, True, 'mkd_sample_masked'),
    ('sample', False, 0.0, False, True, 'mkd_sample_eta'),
    ('sample', False, 0.0, False, False, 'mkd_sample'),
    ('sample_dpmpp', True, 0.0, False, False, 'mkd_sample_dpmpp_ex'),
    ('sample_dpmpp', False, 0.7, True, False, 'mkd_sample_dpmpp_ex'),
    ('sample_dpmpp', False, 0.0, True, False, 'mkd_sample_dpmpp'),
    ('sample_dpmpp', False, 0.0, False, False, 'mkd_sample_dpmpp'),
    ('sample_unipc', True, 0.0, False, False, 'mkd_sample_unipc_ex'),
    ('sample_unipc', False, 0.7, False, False, 'mkd_sample_unipc_ex'),
    ('sample_unipc', False, 0.0, False, False, 'mkd_sample_unipc'),
    ('sample_unipc', False, 0.0, True, False, 'mkd_sample_unipc'),          # (the library refuses the mask: MkdError)
    ('sample_unipc', True, 0.0, True, False, 'mkd_sample_unipc_ex'),
]


@pytest.mark.parametrize('method,trace,phi,masked,eta,entry', LOOP_ENTRIES)
@pytest.mark.parametrize('use_graph', [False, True])
def test_each_option_combination_reaches_its_exported_entry(recorded, method, trace, phi, masked, eta, entry, use_graph):
    """Two steps, batch 2, the 8x8 latent of this file's golden inputs (the size this net runs at throughout the file); a guidance
    rescale needs the guided batch [uncond; cond]."""
    from makeupdiffuse_amd.lib import MkdError
    eng, g, rec = recorded
    sch = sampler.Schedule().make_ddim(5, 0.5 if eta else 0.0)
    n = 2
    tables = [sch.ddim_timesteps[:n], sch.ddim_alphas[:n], sch.ddim_alphas_prev[:n]]
    if method == 'sample':
        tables.append(sch.ddim_sqrt_one_minus_alphas[:n])
    x = g['x']
    gen = torch.Generator().manual_seed(7)
    kw = dict(use_graph=use_graph)
    if phi:
        eng.prepare(torch.cat([g['hint'], g['hint']]), torch.cat([g['uctx'], g['ctx']]))
        kw.update(cfg_scale=9.0, guidance_rescale=phi)
    else:
        eng.prepare(g['hint'], g['ctx'])
    if trace:
        kw.update(want_trace=True, log_every_t=1)
    if masked:
        mask = torch.zeros(1, 1, 8, 8)
        mask[..., :4] = 1.0
        kw.update(x0=torch.randn(x.shape, generator=gen), mask=mask, q_sqrt_ac=[0.9, 0.8][:n], q_sqrt_1m_ac=[0.4, 0.6][:n],
                  q_noise=torch.randn((n, *x.shape), generator=gen))
    if eta:
        kw.update(sigmas=[0.0, float(sch.ddim_sigmas[1])], noise=torch.randn((n, *x.shape), generator=gen))
    rec.calls.clear()
    if method == 'sample_unipc' and masked:
        with pytest.raises(MkdError):
            getattr(eng, method)(x, *tables, **kw)
    else:
        out = getattr(eng, method)(x, *tables, **kw)
        lat = out[0] if trace else out
        assert tuple(lat.shape) == tuple(x.shape) and bool(torch.isfinite(lat).all())
        if trace:
            assert len(out) == 3 and out[1].shape[0] == out[2].shape[0] == n and torch.equal(out[1][-1], lat)
    assert rec.calls == [entry]


@pytest.mark.parametrize('step', ['ddim_step', 'dpmpp_step', 'unipc_step'])
@pytest.mark.parametrize('guided,phi', [(False, 0.0), (False, 0.7), (True, 0.0), (True, 0.7)])
def test_step_calls_use_the_ex_entry_exactly_with_an_engaged_rescale(recorded, step, guided, phi):
    eng, g, rec = recorded
    gen = torch.Generator().manual_seed(8)
    x, e_c = g['x'], torch.randn(g['x'].shape, generator=gen)
    e_u = torch.randn(g['x'].shape, generator=gen) if guided else None
    scale = 9.0 if guided else 1.0
    rec.calls.clear()
    if step == 'ddim_step':
        out = eng.ddim_step(x, e_c, e_u, scale, 0.5, 0.6, 0.0, 0.5 ** 0.5, guidance_rescale=phi)
    elif step == 'dpmpp_step':
        out = eng.dpmpp_step(x, e_c, e_u, scale, [1.4, 0.7, 0.9, 0.3, 0.0, 0.0], guidance_rescale=phi)
    else:
        out = eng.unipc_step(x, None, e_c, e_u, scale, [1.4, 0.7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.9, 0.3, 0.0, 0.0, 0.0], guidance_rescale=phi)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    assert rec.calls == ['mkd_' + step + ('_ex' if guided and phi else '')]


# step_launches(use_graph, cfg, rescale) / (use_graph, cfg, per_sample=True) and eps_launches() of this net prepared with batch 2, read
# from the commit before the engine's loop and step methods shared one call path: no launch was added or removed
LAUNCHES = {'eps': 412,
            ('rows', False, False): 406, ('rows', False, True): 407, ('rows', True, False): 406, ('rows', True, True): 407,
            (False, False, False): 407, (False, False, True): 407, (False, True, False): 408, (False, True, True): 409,
            (True, False, False): 406, (True, False, True): 406, (True, True, False): 407, (True, True, True): 408}


def test_launch_counts_are_those_before_the_shared_call_path(recorded):
    eng, g, _ = recorded
    eng.prepare(g['hint'], g['ctx'])
    got = {'eps': eng.eps_launches()}
    for ug in (False, True):
        for cfg in (False, True):
            got[('rows', ug, cfg)] = eng.step_launches(ug, cfg, per_sample=True)
            for rescale in (False, True):
                got[(ug, cfg, rescale)] = eng.step_launches(ug, cfg, rescale)
    print(got)
    assert got == LAUNCHES
