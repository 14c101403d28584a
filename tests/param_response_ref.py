"""CPU only: the per-tensor response measurement of the engine tests (tests/test_gpu_param_response.py, checked without a GPU by
tests/test_param_response_host.py).

One weight tensor k of the small fixture model is moved along d_k = sd_b[k] - sd[k] (sd_b: an independent redraw of every tensor) by
a_k d_k, and the CHANGE of eps is compared between the fp32 oracle (delta_ref) and the engine (delta_eng): the gain
c_k = <delta_eng, delta_ref> / <delta_ref, delta_ref> is 1 for a correctly wired tensor and about 0 for one that is ignored, dropped or
applied in another tensor's place, and only the component of the engine's bf16 noise along delta_ref enters it.  a_k comes from the rung
table tests/golden/small_param_loud.json, written by tests/make_param_loud.py from the oracle alone."""
import json
import math
import os
import re

import numpy as np
import torch

from oracle import nets, sampler

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TABLE_PATH = os.path.join(GOLD, 'small_param_loud.json')
SMALL = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
             hint_widths=(16, 16, 32, 32, 32, 32, 64))          # tests/test_gpu_engine.py's SMALL
REDRAW = 12345              # sd_b = init_state_dict(cfg, seed + REDRAW)
LADDER = (1, 4, 16, 64, 256, 1024)
RHO_LOUD = 0.2              # the smallest rung with rho = |delta_ref| / |eps_ref| >= RHO_LOUD ...
RHO_SATURATED = 0.8         # ... or, where a normalisation caps rho below that, the smallest with rho >= 0.8 x the ladder's largest
RHO_FLOOR = 0.04            # a condition on the table, not a measurement
NOISE_FACTOR = 1.5          # a rung > 1 is rejected when the bf16-matrix emulation is this much noisier on the loud dict than on the base
TAU_FACTOR = 8.0            # the emulation rounds only the matrices; the engine also rounds activations at every layer boundary
TAU_CAP = 0.5               # an ignored or swapped tensor (c about 0) fails whatever was measured
GROUP_MAX = 20
EPS_REL, EPS_COS = 2e-2, 0.9995          # check_eps of tests/test_gpu_engine.py: the suite's global check


def small_cfg():
    return nets.NetConfig(**SMALL)


def golden_inputs():
    """(seed of the weights, {x, t, hint, ctx, eps}) of tests/golden/small_eps.npz"""
    g = np.load(os.path.join(GOLD, 'small_eps.npz'))
    return int(g['seed_weights']), {k: torch.from_numpy(g[k]) for k in ('x', 't', 'hint', 'ctx', 'eps')}


def state_dicts(cfg, seed):
    return nets.init_state_dict(cfg, seed=seed), nets.init_state_dict(cfg, seed=seed + REDRAW)


def oracle(sd, cfg, G):
    return sampler.apply_model(sd, cfg, G['x'], G['t'], {'c_crossattn': [G['ctx']], 'c_concat': [G['hint']]})


def loud(sd, sd_b, k, a):
    """sd with sd[k] + a (sd_b[k] - sd[k]) in place of sd[k] (a shallow copy: every other tensor is shared)"""
    out = dict(sd)
    out[k] = sd[k] + float(a) * (sd_b[k] - sd[k])
    return out


def gain(d_eng, d_ref):
    """(c, r): the component of the engine's response along the reference's, and the relative residual"""
    d_eng = d_eng.double().flatten().cpu(); d_ref = d_ref.double().flatten().cpu()
    n2 = float(d_ref @ d_ref)
    return float(d_eng @ d_ref) / n2, float((d_eng - d_ref).norm()) / math.sqrt(n2)


def rel_l2(out, ref):
    return float((out.double() - ref.double()).norm() / ref.double().norm())


def global_check_passes(out, ref):
    """check_eps of tests/test_gpu_engine.py as a predicate"""
    out = out.float(); ref = ref.float()
    c = float(torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0))
    return bool(torch.isfinite(out).all()) and rel_l2(out, ref) <= EPS_REL and c >= EPS_COS


def tau(emulated_worst):
    return min(TAU_CAP, TAU_FACTOR * float(emulated_worst))


# ---- the emulated engine: the oracle on weights whose matrices (every tensor of rank >= 2) are rounded to bf16 ------------------
def bf16_matrices(sd, only=None):
    """only: round just these names again (the other entries of sd are taken as already rounded)"""
    out = dict(sd)
    for k in (sd if only is None else only):
        if sd[k].dim() >= 2:
            out[k] = sd[k].to(torch.bfloat16).float()
    return out


class Emulation:
    """engine(sd') for a dict that differs from the base in a few tensors: rounds only those again"""

    def __init__(self, sd, cfg, G):
        self.cfg, self.G = cfg, G
        self.base_sd = bf16_matrices(sd)
        self.base = oracle(self.base_sd, cfg, G)

    def __call__(self, changed):
        """changed: {name: fp32 tensor} in place of the base's"""
        sd = dict(self.base_sd)
        sd.update(changed)
        return oracle(bf16_matrices(sd, only=changed), self.cfg, self.G)


# ---- mutants: each maps the dict the engine was GIVEN to the dict a wrongly wired engine would COMPUTE with ---------------------
def swapped(sd, k1, k2):
    out = dict(sd)
    out[k1], out[k2] = sd[k2], sd[k1]
    return out


def zeroed(sd, k):
    """a dropped bias, a LayerNorm beta that is not folded into its consumer's bias"""
    out = dict(sd)
    out[k] = torch.zeros_like(sd[k])
    return out


SWAP_FAMILIES = (('in_layers.2.bias', 'out_layers.3.bias'), ('norm2.bias', 'norm3.bias'), ('ff.net.2.bias', 'proj_out.bias'),
                 ('emb_layers.1.bias', 'in_layers.2.bias'))
# no fault: conv1's bias and the time-embedding projection's bias are added to the same channel of the same tensor, in either order
SWAP_IS_THE_SAME_FUNCTION = 'emb_layers.1.bias <-> in_layers.2.bias'


def swap_pairs(spec):
    """{family: [(k1, k2)]}: every same-shape neighbour pair that exists in the model"""
    out = {}
    for s1, s2 in SWAP_FAMILIES:
        pairs = []
        for k in sorted(spec):
            if not k.endswith('.' + s1):
                continue
            stem = k[:-len(s1)]
            if s2 == 'proj_out.bias':               # <st>.transformer_blocks.0.ff.net.2.bias <-> <st>.proj_out.bias
                stem = stem[:stem.index('transformer_blocks.')]
            k2 = stem + s2
            if k2 in spec and spec[k2] == spec[k]:
                pairs.append((k, k2))
        out[f'{s1} <-> {s2}'] = pairs
    zc = sorted((k for k in spec if re.search(r'zero_convs\.\d+\.0\.bias$', k)), key=lambda k: int(k.split('.')[-3]))
    zc.append(zc[0].split('zero_convs')[0] + 'middle_block_out.0.bias')
    out['zero-conv bias i <-> i + 1'] = [(a, b) for a, b in zip(zc, zc[1:]) if spec[a] == spec[b]]
    return out


def dropped_biases(spec):
    """every bias that is not a norm's beta"""
    return [k for k in sorted(spec) if k.endswith('.bias') and not is_norm_param(k)]


def ln_betas(spec):
    return [k for k in sorted(spec) if re.search(r'\.norm[123]\.bias$', k)]


# ---- names --------------------------------------------------------------------------------------------------------------------
def is_groupnorm_param(k):
    return bool(re.search(r'(in_layers\.0|out_layers\.0|\.1\.norm|diffusion_model\.out\.0)\.(weight|bias)$', k))


def is_norm_param(k):
    return is_groupnorm_param(k) or bool(re.search(r'\.norm[123]\.(weight|bias)$', k))


def block_of(k):
    """'control_model.input_blocks.4.1', 'model.diffusion_model.middle_block.1', 'control_model.zero_convs', ..."""
    for net in (nets.UNET_PREFIX, nets.CONTROL_PREFIX):
        if k.startswith(net):
            parts = k[len(net):].split('.')
            if parts[0] in ('input_blocks', 'output_blocks'):
                return net + '.'.join(parts[:3])
            if parts[0] == 'middle_block':
                return net + '.'.join(parts[:2])
            return net + parts[0]
    raise KeyError(k)


def groups(names, max_size=GROUP_MAX):
    """[(group id, [names])]: by block prefix, a block of more than max_size tensors in equal consecutive parts"""
    by = {}
    for k in sorted(names):
        by.setdefault(block_of(k), []).append(k)
    out = []
    for b in sorted(by):
        ks = by[b]
        n = -(-len(ks) // max_size)
        per = -(-len(ks) // n)
        for i in range(n):
            out.append((b if n == 1 else f'{b}#{i}', ks[i * per:(i + 1) * per]))
    return out


# the tensors whose derived copies or launches a plan switch changes (the default plan covers every tensor)
def _ends(*suffixes):
    return lambda k: k.endswith(suffixes)


def _feeds_a_groupnorm(k):
    """the producer's epilogue accumulates the statistics after its bias: the biases of the convolutions (the hint block's last one:
    its output is added to conv_in's), of the time-embedding projections and of the merged ff.net.2 + proj_out"""
    if not k.endswith('.bias') or is_norm_param(k) or 'time_embed' in k:
        return False
    if 'input_hint_block' in k:
        return k.endswith('input_hint_block.14.bias')
    return not k.endswith(('to_out.0.bias', 'ff.net.0.proj.bias', 'proj_in.bias'))


VARIANT_TENSORS = {
    # MKD_LN_FLY: LayerNorm 1/2/3 as kernels in front of the plain q|k|v, to_q and interleaved GEGLU weights (0) or folded into them (7)
    'ln_fly': lambda k: bool(re.search(r'\.norm[123]\.(weight|bias)$', k)) or k.endswith(
        ('.attn1.to_q.weight', '.attn1.to_k.weight', '.attn1.to_v.weight', '.attn2.to_q.weight', '.ff.net.0.proj.weight', '.ff.net.0.proj.bias')),
    # skip_fold = 0: conv2 and the 1x1 skip as two launches instead of one GEMM over [W_conv2 | W_skip] with the summed bias
    'skip_fold': _ends('.out_layers.3.weight', '.out_layers.3.bias', '.skip_connection.weight', '.skip_connection.bias'),
    # MKD_GN_FUSED=1: every GroupNorm's gamma and beta, and every bias that enters a tensor a GroupNorm reads
    'gn_fused': lambda k: is_groupnorm_param(k) or _feeds_a_groupnorm(k),
    # MKD_MERGE_FFOUT=0: ff.net.2 and proj_out as two GEMMs instead of the merged one
    'merge_ffout': _ends('.ff.net.2.weight', '.ff.net.2.bias', '.proj_out.weight', '.proj_out.bias'),
}


def variant_names(variant, spec):
    names = [k for k in sorted(spec) if VARIANT_TENSORS[variant](k)]
    if variant == 'skip_fold':
        names = [k for k in names if re.sub(r'\.(out_layers\.3|skip_connection)\.(weight|bias)$', '', k) + '.skip_connection.weight' in spec]
    return names


# ---- the rung table -----------------------------------------------------------------------------------------------------------
def load_table(path=TABLE_PATH):
    """{'emulated_worst_gain_error': float, 'one_rung_down': {name: reason}, 'tensors': {name: (a, rho)}}"""
    with open(path) as f:
        t = json.load(f)
    t['tensors'] = {k: (int(a), float(rho)) for k, (a, rho) in t['tensors'].items()}
    return t


def choose_rung(rho, admissible):
    """rho(i), admissible(i): callables per rung index of LADDER (evaluated only where the rule needs them).  The smallest rung with
    rho >= RHO_LOUD, else the smallest with rho >= RHO_SATURATED x the ladder's largest; if that rung is not admissible, the admissible
    rung BELOW it of the largest rho (a = 1 always is admissible).  Not a rung above it: what makes a rung noisy is a softmax
    that the amplified tensor (to_q, to_k, norm1) saturates, and a larger factor saturates it further - where the emulation is quiet
    again up there, the softmax has become a hard arg-max, stable under rounded MATRICES but flipped by the rounding of the scores
    themselves, which the emulation does not model (on the device those rungs are 0.04 to 0.28 from the oracle in rel-L2)."""
    n = len(LADDER)
    i = next((j for j in range(n) if rho(j) >= RHO_LOUD), None)
    if i is None:
        top = max(rho(j) for j in range(n))
        i = min(j for j in range(n) if rho(j) >= RHO_SATURATED * top)
    if not admissible(i):
        i = max((j for j in range(i) if admissible(j)), key=rho)
    return i
