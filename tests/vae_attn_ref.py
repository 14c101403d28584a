"""float64 restatement of the first-stage mid-block attention as a STAGE (mkd_ctx::vae_attn, reached through
mkd_debug_vae_attn), the cases tests/test_gpu_vae_attn.py runs, and a torch emulation of the two orders of rounding the scores can
take (test infrastructure only; written from oracle/vae.py `_attn` and the comments of vae_attn).

The stage holds bf16 tensors in four places: the weights, the GroupNorm output, q|k and V^T.  `stage` rounds there and nowhere else:
scores, softmax, P.V, the v bias, proj_out and the residual are exact, so that what the device adds (fp32 scores, bf16
probabilities, bf16 o, bf16 out, MFMA accumulation order) is measured against it.  The v bias is added after P.V, as the engine does
(softmax rows sum to 1).

Bounds of the GPU test, on o and on out: assert_close_bf16 (rel-L2 <= 4e-3, max-abs <= 2^-6 |ref|_inf) and per-row rel-L2 <= 8e-3
over every row.  tests/test_vae_attn_ref_host.py shows that `emulate(..., scores='fp32')` stays inside them on every case and that
`scores='bf16'` leaves them on every case with logit std >= 4."""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from oracle import vae

Tensor = torch.Tensor

REL_WHOLE = 4e-3            # gpu_util.assert_close_bf16
MAXABS = 2.0 ** -6          # ... x |ref|_inf
REL_ROW = 8e-3              # per output row, no row left out

# net: 'small' (ch 32, ch_mult (1, 2): mid width 64) or 'real' (ch 128, ch_mult (1, 4): mid width 512); which: 'dec' / 'enc';
# s multiplies q.weight and k.weight (logit std about s^2); spike: one token of x times 6
Case = namedtuple('Case', 'net which B H W s spike')
NETS = {'small': vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2), num_res_blocks=1, out_ch=3),
        'real': vae.VaeConfig(z_channels=4, embed_dim=4, ch=128, ch_mult=(1, 4), num_res_blocks=1, out_ch=3)}
SCALES = (1, 2, 3)


def width(net: str) -> int:
    c = NETS[net]
    return c.ch * c.ch_mult[-1]


def cases():
    out = []
    for which in ('dec', 'enc'):
        for B, H, W in ((2, 16, 16), (3, 4, 12), (1, 32, 32)):
            out += [Case('small', which, B, H, W, s, False) for s in SCALES]
    for B, H, W in ((1, 8, 8), (2, 16, 16)):
        out += [Case('real', 'dec', B, H, W, s, False) for s in SCALES]
    out.append(Case('small', 'dec', 2, 16, 16, 2, True))
    return out


def case_id(c: Case) -> str:
    return f'{c.net}-{c.which}-{c.B}x{c.H}x{c.W}-s{c.s}' + ('-spike' if c.spike else '')


def prefix(which: str) -> str:
    return vae.PREFIX + ('decoder.' if which == 'dec' else 'encoder.') + 'mid.attn_1'


_sd_cache = {}


def state_dict(net: str, which: str) -> Dict[str, Tensor]:
    """Seeded weights of the whole decoder / encoder of `net` (what the engine loads), unscaled; one per (net, which), not to be modified."""
    if (net, which) not in _sd_cache:
        if which == 'dec':
            _sd_cache[net, which] = vae.init_state_dict(NETS[net], seed=31)
        else:
            try:
                import vae_encoder_ref as enc_ref
            except ImportError:
                from tests import vae_encoder_ref as enc_ref
            _sd_cache[net, which] = enc_ref.init_state_dict(NETS[net], seed=32)
    return _sd_cache[net, which]


def scale_qk(sd: Dict[str, Tensor], p: str, s: float) -> Dict[str, Tensor]:
    """A copy of sd with q.weight and k.weight of the attention at p multiplied by s."""
    sd = dict(sd)
    for n in ('q', 'k'):
        sd[f'{p}.{n}.weight'] = sd[f'{p}.{n}.weight'] * s
    return sd


def make_x(c: Case) -> Tensor:
    """bf16 NHWC [B, H, W, C]: randn plus a per-channel offset in [-1, 1]; spiked: token (0, H/2, W/3) times 6."""
    C = width(c.net)
    g = torch.Generator().manual_seed(1000 * c.B + 10 * c.H + c.W + C)
    x = torch.randn(c.B, c.H, c.W, C, generator=g) + (torch.rand(C, generator=g) * 2 - 1)
    if c.spike:
        x[0, c.H // 2, c.W // 3] *= 6
    return x.to(torch.bfloat16)


def q16(t: Tensor) -> Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _parts(sd, p, x_nhwc: Tensor, rounding: bool):
    """(x [B,T,C], g, q, k, v without bias, Wp, scale) in float64, rounded to bf16 where the stage holds bf16 tensors."""
    r = (lambda t: q16(t.float()).double()) if rounding else (lambda t: t.double())
    B, H, W, C = x_nhwc.shape
    x = x_nhwc.double().reshape(B, H * W, C)
    gn = F.group_norm(x.transpose(1, 2), 32, sd[f'{p}.norm.weight'].double(), sd[f'{p}.norm.bias'].double(), eps=1e-6).transpose(1, 2)
    g = r(gn)
    w = {n: r(sd[f'{p}.{n}.weight'].reshape(C, C)) for n in ('q', 'k', 'v', 'proj_out')}
    b = {n: sd[f'{p}.{n}.bias'].double() for n in ('q', 'k', 'v', 'proj_out')}
    q = r(g @ w['q'].T + b['q'])
    k = r(g @ w['k'].T + b['k'])
    v = r(g @ w['v'].T)                                   # V^T in the engine: bias-free, bf16
    return x, q, k, v, w['proj_out'], b, float(C) ** -0.5


def stage(sd: Dict[str, Tensor], p: str, x_nhwc: Tensor, rounding: bool = True) -> Tuple[Tensor, Tensor, dict]:
    """o [B*T, C], out [B, H, W, C] (float64) and {'logit_std', 'logit_max'} of the scaled scores."""
    B, H, W, C = x_nhwc.shape
    x, q, k, v, wp, b, scale = _parts(sd, p, x_nhwc, rounding)
    s = (q @ k.transpose(1, 2)) * scale
    o = torch.softmax(s, -1) @ v + b['v']
    out = x + o @ wp.T + b['proj_out']
    return o.reshape(B * H * W, C), out.reshape(B, H, W, C), {'logit_std': s.std().item(), 'logit_max': s.abs().max().item()}


def emulate(sd: Dict[str, Tensor], p: str, x_nhwc: Tensor, scores: str = 'fp32') -> Tuple[Tensor, Tensor]:
    """The stage with the roundings a device pipeline adds: scores held as `scores` ('fp32' or 'bf16'), probabilities, o and out
    rounded to bf16 (sums in float64: accumulation order is not what is being told apart)."""
    B, H, W, C = x_nhwc.shape
    x, q, k, v, wp, b, scale = _parts(sd, p, x_nhwc, True)
    s = ((q @ k.transpose(1, 2)) * scale).float()
    s = (q16(s) if scores == 'bf16' else s).double()
    pr = q16(torch.softmax(s, -1).float()).double()
    o = q16((pr @ v + b['v']).float()).double()
    out = q16((x + o @ wp.T + b['proj_out']).float()).double()
    return o.reshape(B * H * W, C), out.reshape(B, H, W, C)


def measures(got: Tensor, ref: Tensor) -> dict:
    """whole rel-L2, max-abs / |ref|_inf and the worst row's rel-L2 (rows = tokens, over the last dim)."""
    got = got.double().reshape(-1, got.shape[-1]); ref = ref.double().reshape(-1, ref.shape[-1])
    d = got - ref
    return {'whole': (d.norm() / ref.norm()).item(), 'maxabs': (d.abs().max() / ref.abs().max()).item(),
            'row': (d.norm(dim=1) / ref.norm(dim=1)).max().item()}


def inside(m: dict) -> bool:
    return m['whole'] <= REL_WHOLE and m['maxabs'] <= MAXABS and m['row'] <= REL_ROW
