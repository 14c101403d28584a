"""No GPU: the per-tensor response check of tests/test_gpu_param_response.py earns its place, shown on the emulated engine of
tests/param_response_ref.py (the oracle on bf16-rounded matrices).  The committed rung table is the generator's (keys, rho of every
tensor, the rung rule re-run on every 16th tensor, the rho floor, the recorded emulated worst gain error); the correctly wired
emulation passes the device test's assertions on all 664 tensors; every wiring fault below, run as "the engine" through the same
assertions, is flagged by the gain criterion on EVERY case, while the suite's global check (check_eps: rel-L2 <= 2e-2 and
cosine >= 0.9995 on the final eps of the base dict) passes most of them.  As printed by test_every_mutant_is_flagged_by_the_gain
(cases = every tensor, or every same-shape neighbour pair, that exists in the small model; "flagged" = |c - 1| > tau):

  fault (the emulated engine computes with ...)      flagged by the gain      |c - 1| of the cases       the global check passes
  reloaded tensor ignored                            664 of 664 tensors       1                          664 of 664
  swapped in_layers.2.bias <-> out_layers.3.bias      36 of  36 (18 pairs)    0.149 .. 1.98               16 of  18 pairs
  swapped norm2.bias <-> norm3.bias                   32 of  32 (16 pairs)    0.214 .. 2.14                0 of  16
  swapped ff.net.2.bias <-> proj_out.bias             32 of  32 (16 pairs)    0.507 .. 1.20               16 of  16
  swapped zero-conv bias i <-> i + 1                  10 of  10 (5 pairs)     0.115 .. 1.41                4 of   5
  bias dropped (every bias that is no norm's beta)   183 of 183               1                          150 of 183
  LayerNorm beta not folded (norm1/2/3.bias)          48 of  48               1                           16 of  48
  swapped emb_layers.1.bias <-> in_layers.2.bias       0 of  36 (18 pairs)    <= 0.002                    18 of  18
tau = 8 x 0.00585 = 0.0468 (the correctly wired emulation: worst |c - 1| 0.00585, worst residual r 0.038, rel-L2 7.4e-3 on the base dict
and <= 1.09e-2 on a loud dict); the nearest fault is 2.4 tau away.  The last row is no fault and must NOT be flagged: conv1's bias and the
time-embedding projection's bias are added to the same channel of the same tensor, so swapping them is the same function.  "Ignored",
"dropped" and "not folded" respond with exactly 0 to the reload, whatever the tensor; the global check on the base dict cannot see an
ignored reload at all, passes 82 % of the dropped biases and every ff.net.2.bias / proj_out.bias swap (the pair the load-time merge folds
into one vector).  It does see every norm2 / norm3 beta swap: the fixture's betas are drawn with sigma 0.2.
"""
import pytest
import torch

from oracle import nets
from tests import make_param_loud as M
from tests import param_response_ref as R

CFG = R.small_cfg()
SPEC = nets.full_param_spec(CFG)
TABLE = R.load_table()
TAU = R.tau(TABLE['emulated_worst_gain_error'])


@pytest.fixture(scope='module')
def world():
    """the full 664-tensor emulation, once: per tensor the oracle's and the emulated engine's eps on the loud dict"""
    torch.set_num_threads(min(4, torch.get_num_threads()))
    seed, G = R.golden_inputs()
    sd, sd_b = R.state_dicts(CFG, seed)
    w = dict(G=G, sd=sd, sd_b=sd_b, base=R.oracle(sd, CFG, G), emu=R.Emulation(sd, CFG, G), w={}, ref={}, eng={})
    for k in sorted(sd):
        sd1 = R.loud(sd, sd_b, k, TABLE['tensors'][k][0])
        w['w'][k] = sd1[k]
        w['ref'][k] = R.oracle(sd1, CFG, G)
        w['eng'][k] = w['emu']({k: sd1[k]})
    return w


def test_table_keys_groups_and_variants_cover_the_model():
    assert set(TABLE['tensors']) == set(SPEC) and tuple(TABLE['ladder']) == R.LADDER
    assert all(a in R.LADDER for a, _ in TABLE['tensors'].values())
    gs = R.groups(SPEC)
    assert sorted(k for _, names in gs for k in names) == sorted(SPEC)          # the union of the groups is the key set, no tensor twice
    assert max(len(names) for _, names in gs) <= R.GROUP_MAX
    for v in R.VARIANT_TENSORS:
        names = R.variant_names(v, SPEC)
        assert names and set(names) <= set(SPEC), v
    assert set(TABLE['one_rung_down']) == set(M.ONE_RUNG_DOWN)


def test_every_rho_is_the_tables_and_above_the_floor(world):
    assert torch.allclose(world['base'], world['G']['eps'], rtol=0, atol=1e-5)
    for k, (a, rho_t) in TABLE['tensors'].items():
        rho = float((world['ref'][k] - world['base']).norm() / world['base'].norm())
        assert abs(rho - rho_t) <= 1e-3 * rho_t, (k, a, rho, rho_t)
        assert rho_t >= R.RHO_FLOOR, f'{k}: rho {rho_t} below the floor: regenerate the table'


def test_the_rung_rule_gives_the_tables_rung_on_every_16th_tensor(world):
    for k in sorted(SPEC)[::16]:
        i, rho, *_ = M.rung_of(k, world['sd'], world['sd_b'], CFG, world['G'], world['base'], world['emu'])
        a_t, rho_t = TABLE['tensors'][k]
        assert R.LADDER[i] == a_t and abs(rho - rho_t) <= 1e-3 * rho_t, (k, R.LADDER[i], rho, a_t, rho_t)


def test_correct_wiring_passes_every_assertion_of_the_device_test(world):
    emu = world['emu']
    base_noise = R.rel_l2(emu.base, world['base'])
    worst, worst_r, worst_rel = (0.0, None), 0.0, 0.0
    for k in sorted(SPEC):
        c, r = R.gain(world['eng'][k] - emu.base, world['ref'][k] - world['base'])
        worst, worst_r = max(worst, (abs(c - 1), k)), max(worst_r, r)
        worst_rel = max(worst_rel, R.rel_l2(world['eng'][k], world['ref'][k]))
        assert R.global_check_passes(world['eng'][k], world['ref'][k]), f'{k}: the loud dict is not an ordinary evaluation any more'
        assert abs(c - 1) <= TAU, (k, c, TAU)
    print(f'emulated engine: base rel-L2 {base_noise:.3e}, worst on a loud dict {worst_rel:.3e}; worst |c-1| {worst[0]:.5f} ({worst[1]}), '
          f'worst r {worst_r:.4f}; tau {TAU:.4f}')
    # the figure tau is taken from is the generator's: fp32 evaluation noise between thread counts is 1.2e-6 |eps| per evaluation,
    # over |d_ref| >= 0.04 |eps| and four evaluations that is 1.2e-4 in c at the most
    assert abs(worst[0] - TABLE['emulated_worst_gain_error']) <= 2e-4, (worst, TABLE['emulated_worst_gain_error'])
    assert 0 < TAU <= R.TAU_CAP


def test_every_mutant_is_flagged_by_the_gain(world):
    sd, emu, base = world['sd'], world['emu'], world['base']
    rows = []

    def row(name, cs, passes, fault=True):
        flagged = sum(1 for c in cs if abs(c - 1) > TAU)
        rows.append(f'  {name:47s} flagged on {flagged:3d} of {len(cs):3d}, |c - 1| in [{min(abs(c - 1) for c in cs):.4f}, '
                    f'{max(abs(c - 1) for c in cs):.3f}]   the global check passes {sum(passes):3d} of {len(passes):3d}')
        assert flagged == (len(cs) if fault else 0), (name, [c for c in cs if (abs(c - 1) <= TAU) == fault])

    # the reloaded tensor is ignored: the engine goes on computing with the base dict, which is right on the base dict
    row('reloaded tensor ignored', [R.gain(emu.base - emu.base, world['ref'][k] - base)[0] for k in sorted(SPEC)], [True] * len(SPEC))
    # two same-shape neighbours swapped: what is loaded as k1 is applied as k2 and the other way round
    for family, pairs in R.swap_pairs(SPEC).items():
        cs, passes = [], []
        for k1, k2 in pairs:
            wrong_base = emu({k1: sd[k2], k2: sd[k1]})
            passes.append(R.global_check_passes(wrong_base, base))
            for ka, kb in ((k1, k2), (k2, k1)):
                out = emu({kb: world['w'][ka], ka: sd[kb]})
                cs.append(R.gain(out - wrong_base, world['ref'][ka] - base)[0])
        row(f'swapped {family}', cs, passes, fault=family != R.SWAP_IS_THE_SAME_FUNCTION)
    # a bias dropped / a LayerNorm beta not folded into its consumer's bias: zero is used whatever is loaded, so the response is exactly 0
    for name, ks in (('bias dropped', R.dropped_biases(SPEC)), ('LayerNorm beta not folded', R.ln_betas(SPEC))):
        passes = [R.global_check_passes(emu({k: torch.zeros_like(sd[k])}), base) for k in ks]
        row(name, [0.0] * len(ks), passes)
    print('\n' + '\n'.join(rows))
