"""Writes tests/golden/small_param_loud.json, the rung table of tests/param_response_ref.py, from the CPU oracle alone
(a few CPU-minutes; run once, commit the output):

    python tests/make_param_loud.py

Per tensor k of the small fixture model: the rung a_k of LADDER that makes the tensor loud (param_response_ref.choose_rung), and
rho_k = |oracle(sd'_k) - oracle(sd)| / |oracle(sd)| at that rung.  A rung above 1 is admissible only if the emulated engine (the oracle on
bf16-rounded matrices) is at most NOISE_FACTOR x as far from the oracle on the loud dict as on the base dict.  ONE_RUNG_DOWN lists the
tensors that a device run showed to be too hard for bf16 at the rule's rung, with the reason; rho_k >= RHO_FLOOR holds for them too.
Also recorded: the worst |c_k - 1| of the emulated engine at the chosen rungs, from which the device test takes its tolerance
(tests/test_param_response_host.py recomputes both the table and that figure)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import param_response_ref as R  # noqa: E402

# name -> why the tensor sits one rung below the rule's choice
ONE_RUNG_DOWN = {
    'model.diffusion_model.output_blocks.2.1.transformer_blocks.0.attn1.to_k.weight':
        'to_k x 16 sharpens the self-attention softmax of a 64-token block: at a = 16 it was the noisiest tensor of the emulation '
        '(|c - 1| 0.0060) and on the device, correctly wired (gain 0.988), its loud dict sat at rel-L2 2.03e-2 under MKD_LN_FLY=0',
}


def rung_of(k, sd, sd_b, cfg, G, base, emu):
    """(index into LADDER, rho there, the emulated engine's eps there, was the rule's rung rejected as noisy)"""
    rho, emu_eps, ref_eps = {}, {}, {}

    def get_rho(i):
        if i not in rho:
            ref_eps[i] = R.oracle(R.loud(sd, sd_b, k, R.LADDER[i]), cfg, G)
            rho[i] = float((ref_eps[i] - base).norm() / base.norm())
        return rho[i]

    def admissible(i):
        get_rho(i)
        if i not in emu_eps:
            emu_eps[i] = emu({k: R.loud(sd, sd_b, k, R.LADDER[i])[k]})
        return i == 0 or R.rel_l2(emu_eps[i], ref_eps[i]) <= R.NOISE_FACTOR * R.rel_l2(emu.base, base)

    first = {}

    def adm_noting(i):
        ok = admissible(i)
        first.setdefault('ok', ok)
        return ok

    i = R.choose_rung(get_rho, adm_noting)
    if k in ONE_RUNG_DOWN:
        assert i > 0, k
        i -= 1
    admissible(i)
    return i, get_rho(i), emu_eps[i], ref_eps[i], not first['ok']


def main():
    torch.set_num_threads(4)
    cfg = R.small_cfg()
    seed, G = R.golden_inputs()
    sd, sd_b = R.state_dicts(cfg, seed)
    base = R.oracle(sd, cfg, G)
    assert torch.allclose(base, G['eps'], rtol=0, atol=1e-5)
    emu = R.Emulation(sd, cfg, G)
    print(f'emulated engine on the base dict: rel-L2 {R.rel_l2(emu.base, base):.3e}')
    tensors, worst, rejected = {}, (0.0, None), []
    for n, k in enumerate(sorted(sd)):
        i, rho, e_eps, r_eps, rej = rung_of(k, sd, sd_b, cfg, G, base, emu)
        c, r = R.gain(e_eps - emu.base, r_eps - base)
        tensors[k] = [R.LADDER[i], float(f'{rho:.6g}')]
        worst = max(worst, (abs(c - 1), k))
        if rej:
            rejected.append(k)
        print(f'{n:3d} {k}: a {R.LADDER[i]} rho {rho:.4f} c-1 {c - 1:+.5f} r {r:.4f}{" (rule rung rejected as noisy)" if rej else ""}', flush=True)
    low = {k: v for k, v in tensors.items() if v[1] < R.RHO_FLOOR}
    assert not low, f'rho below the floor {R.RHO_FLOOR}: {low}'
    out = {'ladder': list(R.LADDER), 'emulated_worst_gain_error': float(f'{worst[0]:.4g}'), 'emulated_worst_tensor': worst[1],
           'noisy_at_the_rule_rung': rejected, 'one_rung_down': ONE_RUNG_DOWN, 'tensors': tensors}
    with open(R.TABLE_PATH, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    counts = {a: sum(1 for v in tensors.values() if v[0] == a) for a in R.LADDER}
    print(f'wrote {R.TABLE_PATH}: rungs {counts}, min rho {min(v[1] for v in tensors.values()):.4f}, '
          f'{len(rejected)} rule rungs rejected, emulated worst |c-1| {worst[0]:.4g} ({worst[1]})')


if __name__ == '__main__':
    main()
