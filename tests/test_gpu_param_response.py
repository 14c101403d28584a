"""-m gpu: every weight tensor's effect on eps, engine against oracle, on the small fixture model (tests/param_response_ref.py).

check_eps sees one global rel-L2 on the final eps: 195 of the 664 tensors move eps by less than its 2e-2 when they are replaced by an
independent redraw, so they could be dropped, swapped with a same-shape neighbour or folded into the wrong launch unnoticed
(tests/test_param_response_host.py has the counts per fault).  Here each tensor k is reloaded ALONE, moved along its redraw direction by
the factor a_k of the committed rung table (chosen on the CPU by the oracle alone so that eps moves by rho_k >= 0.04, mostly >= 0.2, of
its norm), through the single-tensor path load_weight -> finalize -> prepare, which rebuilds every derived weight form (q|k|v and K|V
concatenations, LayerNorm folds, merged ff.net.2 . proj_out, interleaved GEGLU, [W_conv2 | W_skip], the time-embedding tables).  Per tensor:
  1. the loud dict is an ordinary model evaluation: check_eps(engine, oracle) with the suite's budget (rel-L2 <= 2e-2, cos >= 0.9995);
  2. the gain c_k = <d_eng, d_ref> / <d_ref, d_ref> of the CHANGE of eps has |c_k - 1| <= tau;
  3. rho_k, recomputed live, agrees with the table to 1e-3 relative and is >= 0.04.
The first tensor of every group is also loaded into a fresh engine with load_state_dict: bit-equal eps, or a derived copy was stale.  After
the group its tensors are back and eps is bit-equal to the base eps.

tau = 8 x the worst |c_k - 1| of the host emulation (the oracle on bf16-rounded matrices; 8 because the engine also rounds activations
at every layer boundary), never above 0.5.  The emulated worst is recorded in the table by its generator and recomputed by the host test.
  emulated worst |c - 1|   0.00585 (input_blocks.4.1 norm2.bias of the UNet)
  tau                      0.0468
  measured on an MI355X    plan            tensors  worst |c - 1|  worst r  worst rel-L2 on a loud dict
                           default         664      0.0389         0.216    1.95e-2
                           MKD_LN_FLY=0    192      0.0128         0.118    1.98e-2
                           MKD_LN_FLY=7    192      0.0091         0.117    1.95e-2
                           MKD_SKIP_FOLD=0  32      0.0035         0.049    1.44e-2
                           MKD_GN_FUSED=1  214      0.0458         0.220    1.47e-2
                           MKD_MERGE_FFOUT=0 64     0.0059         0.051    1.60e-2
The worst gain is control_model.middle_block.2.in_layers.0.bias in both plans that hold it: a = 16, rho = 0.047, among the quietest
tensors of the table (the ControlNet's last ResBlock reaches eps only through middle_block_out), so
the engine's noise is a fifth of the response (r 0.22) before the projection.  The nearest emulated wiring fault has |c - 1| = 0.115.
One tensor sits one rung below the rule's choice (make_param_loud.ONE_RUNG_DOWN: at a = 16 output_blocks.2.1 attn1.to_k.weight was at
rel-L2 2.03e-2 under MKD_LN_FLY=0 with gain 0.988, rounding on a sharpened softmax).
The whole file takes half a minute on the device; a group takes at most 0.6 s.

Plan variants re-run the tensors whose derived copies or launches the switch changes (param_response_ref.VARIANT_TENSORS) on an engine of
their own: MKD_LN_FLY=0 and =7 (at this size the default plan already takes 7: every transformer has <= 256 rows), MKD_SKIP_FOLD=0,
MKD_GN_FUSED=1, MKD_MERGE_FFOUT=0.  Out of scope: the d = 320 fused transformer tail and head (never engaged at this size), the full-size
model, guidance / interpolation / regions conditioning, VAE, CLIP and parser weights."""
import time

import pytest
import torch
import torch.nn.functional as F

from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from oracle import nets
from tests import param_response_ref as R

pytestmark = pytest.mark.gpu

CFG = R.small_cfg()
SPEC = nets.full_param_spec(CFG)
TABLE = R.load_table()
TAU = R.tau(TABLE['emulated_worst_gain_error'])
# plan -> (environment read when the context is created, the tensors it covers)
PLANS = {
    'default': ({}, sorted(SPEC)),
    'ln_fly0': ({'MKD_LN_FLY': '0'}, R.variant_names('ln_fly', SPEC)),
    'ln_fly7': ({'MKD_LN_FLY': '7'}, R.variant_names('ln_fly', SPEC)),
    'skip_fold0': ({'MKD_SKIP_FOLD': '0'}, R.variant_names('skip_fold', SPEC)),
    'gn_fused': ({'MKD_GN_FUSED': '1'}, R.variant_names('gn_fused', SPEC)),
    'unmerged_ffout': ({'MKD_MERGE_FFOUT': '0'}, R.variant_names('merge_ffout', SPEC)),
}
CASES = {(plan, gid): names for plan, (_, covered) in PLANS.items() for gid, names in R.groups(covered)}


def check_eps(out, ref, what):
    """tests/test_gpu_engine.py's check_eps, the suite's budget"""
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), f'{what}: non-finite'
    r = ((out - ref).norm() / ref.norm()).item()
    c = F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    assert r <= R.EPS_REL and c >= R.EPS_COS, f'{what}: rel-L2 {r:.4e} (<= {R.EPS_REL}), cos {c:.6f} (>= {R.EPS_COS})'
    return r


class Reference:
    """the oracle's side, computed once per tensor and shared by the plans"""

    def __init__(self):
        seed, self.G = R.golden_inputs()
        self.sd, self.sd_b = R.state_dicts(CFG, seed)
        self.base = R.oracle(self.sd, CFG, self.G)
        self._loud = {}

    def loud(self, k):
        """(a_k, the loud tensor, the oracle's eps on the loud dict)"""
        if k not in self._loud:
            a = TABLE['tensors'][k][0]
            sd1 = R.loud(self.sd, self.sd_b, k, a)
            self._loud[k] = (a, sd1[k], R.oracle(sd1, CFG, self.G))
        return self._loud[k]


@pytest.fixture(scope='module')
def ref():
    r = Reference()
    assert torch.allclose(r.base, r.G['eps'], rtol=0, atol=1e-5), 'the oracle no longer gives the golden eps'
    return r


@pytest.fixture(scope='module')
def engines():
    made = {}
    yield made
    for eng, _ in made.values():
        eng.close()


def run(eng, ref):
    eng.finalize()
    eng.prepare(ref.G['hint'], ref.G['ctx'])
    return eng.eps(ref.G['x'], ref.G['t']).cpu()


def engine_of(plan, engines, ref, monkeypatch):
    """one engine per plan, loaded with the base dict; its base eps"""
    for name, value in PLANS[plan][0].items():
        monkeypatch.setenv(name, value)
    if plan not in engines:
        eng = MkdEngine(NetConfig(**R.SMALL))
        assert set(eng.expected_params()) == set(ref.sd)
        eng.load_state_dict(ref.sd)
        base = run(eng, ref)
        check_eps(base, ref.base, f'{plan}: base dict')
        engines[plan] = (eng, base)
    return engines[plan]


def test_the_groups_cover_every_tensor_and_the_variants_their_lists():
    assert set(TABLE['tensors']) == set(SPEC)
    for plan, (_, covered) in PLANS.items():
        got = [k for (p, _), names in CASES.items() if p == plan for k in names]
        assert sorted(got) == sorted(covered) and len(set(got)) == len(got) and got, plan
    n_tfm = sum(1 for k in SPEC if k.endswith('.norm1.weight'))
    n_skip = sum(1 for k in SPEC if k.endswith('.skip_connection.weight'))
    n_gn = sum(1 for k in SPEC if R.is_groupnorm_param(k))
    assert len(PLANS['default'][1]) == len(SPEC) == 664
    assert len(PLANS['ln_fly0'][1]) == 12 * n_tfm and len(PLANS['skip_fold0'][1]) == 4 * n_skip and n_tfm == 16 and n_skip == 8
    assert len(PLANS['unmerged_ffout'][1]) == 4 * n_tfm and n_gn == 106
    assert set(k for k in SPEC if R.is_groupnorm_param(k)) <= set(PLANS['gn_fused'][1]) and len(PLANS['gn_fused'][1]) == 214
    assert 0 < TAU <= R.TAU_CAP and min(rho for _, rho in TABLE['tensors'].values()) >= R.RHO_FLOOR


def test_each_switch_selects_another_plan(engines, ref, monkeypatch):
    """the variants are not the default plan under another name: the launch count of one evaluation moves (MKD_LN_FLY=7 is what the
    default plan takes at this size: same count)"""
    n = {}
    for plan in PLANS:
        with monkeypatch.context() as m:
            n[plan] = engine_of(plan, engines, ref, m)[0].eps_launches()
    print(n)
    assert n['ln_fly7'] == n['default']
    for plan in ('ln_fly0', 'skip_fold0', 'gn_fused', 'unmerged_ffout'):
        assert n[plan] != n['default'], (plan, n)
    assert engines['ln_fly0'][0].get_option('ln_fly') == 0 and engines['skip_fold0'][0].get_option('skip_fold') == 0


@pytest.mark.parametrize('plan,gid', list(CASES), ids=[f'{p}-{g}' for p, g in CASES])
def test_every_tensor_of_the_group_moves_eps_as_in_the_oracle(plan, gid, engines, ref, monkeypatch):
    names = CASES[(plan, gid)]
    t0 = time.time()
    eng, base = engine_of(plan, engines, ref, monkeypatch)
    bad, worst_c, worst_r, worst_rel = [], (0.0, ''), 0.0, 0.0
    try:
        for j, k in enumerate(names):
            a, w, ref_loud = ref.loud(k)
            rho_t = TABLE['tensors'][k][1]
            eng.load_weight(k, w)
            out = run(eng, ref)
            eng.load_weight(k, ref.sd[k])                      # (rebuilt with the next tensor's finalize, or the one after the loop)
            d_ref = ref_loud - ref.base
            rho = float(d_ref.norm() / ref.base.norm())
            c, r = R.gain(out - base, d_ref)
            rel = R.rel_l2(out, ref_loud)
            worst_c, worst_r, worst_rel = max(worst_c, (abs(c - 1), k)), max(worst_r, r), max(worst_rel, rel)
            what = f'{k}: a {a} rho {rho:.4f} (table {rho_t:.4f}) c {c:.4f} r {r:.4f} rel-L2 {rel:.3e}'
            try:
                check_eps(out, ref_loud, 'loud dict')
                assert abs(c - 1) <= TAU, f'gain off by more than tau = {TAU:.4f}'
                assert abs(rho - rho_t) <= 1e-3 * rho_t and rho >= R.RHO_FLOOR, 'rho is not the table\'s'
                if j == 0:                                     # the same dict loaded as a whole into a fresh engine
                    fresh = MkdEngine(NetConfig(**R.SMALL))
                    try:
                        fresh.load_state_dict(R.loud(ref.sd, ref.sd_b, k, a))
                        assert torch.equal(run(fresh, ref), out), 'single-tensor reload differs from a fresh load_state_dict: stale derived copy'
                    finally:
                        fresh.close()
            except AssertionError as e:
                bad.append(f'{what}: {e}')
    finally:
        for k in names:
            eng.load_weight(k, ref.sd[k])
        back = run(eng, ref)
    print(f'[{plan}] {gid}: {len(names)} tensors, worst |c-1| {worst_c[0]:.4f} ({worst_c[1]}; tau {TAU:.4f}), worst r {worst_r:.4f}, '
          f'worst rel-L2 on a loud dict {worst_rel:.3e}, {time.time() - t0:.1f} s')
    assert not bad, '\n'.join(bad)
    assert torch.equal(back, base), 'the restored weights do not give the base eps bit for bit'
