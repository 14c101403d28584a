"""Python host wrapper of the libmkd engine (plumbing: torch supplies device memory and the stream).

``MkdEngine`` is what ``diffmk.makeup_diffuse`` model classes delegate ``apply_model`` / ``sample_log``
to.  Everything here fails loudly without a GPU or without libmkd.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib
from .sampling import SOLVERS as _SOLVER


@dataclass
class NetConfig:
    """control_stage_config / unet_config params of diffmodels/base_diffusion_makeup.yaml:52-84."""
    in_channels: int = 4
    out_channels: int = 4
    hint_channels: int = 6
    model_channels: int = 320
    attention_resolutions: Sequence[int] = (4, 2, 1)
    num_res_blocks: int = 2
    channel_mult: Sequence[int] = (1, 2, 4, 4)
    num_heads: int = 8
    transformer_depth: int = 1
    context_dim: int = 768
    hint_widths: Sequence[int] = (16, 16, 32, 32, 96, 96, 256)

    @classmethod
    def from_yaml_params(cls, control: dict, unet: dict) -> 'NetConfig':
        for k in ('model_channels', 'attention_resolutions', 'num_res_blocks', 'channel_mult', 'num_heads',
                  'transformer_depth', 'context_dim', 'in_channels'):
            if k in control and k in unet and list(np.atleast_1d(control[k])) != list(np.atleast_1d(unet[k])):
                raise ValueError(f'control_stage_config and unet_config disagree on {k}')
        if not unet.get('use_spatial_transformer', True) or unet.get('legacy', False):
            raise NotImplementedError('only use_spatial_transformer=True, legacy=False is supported')
        return cls(in_channels=unet.get('in_channels', 4), out_channels=unet.get('out_channels', 4),
                   hint_channels=control.get('hint_channels', 6), model_channels=unet['model_channels'],
                   attention_resolutions=tuple(unet['attention_resolutions']),
                   num_res_blocks=unet['num_res_blocks'], channel_mult=tuple(unet['channel_mult']),
                   num_heads=unet['num_heads'], transformer_depth=unet.get('transformer_depth', 1),
                   context_dim=unet['context_dim'],
                   hint_widths=tuple(control.get('hint_widths', (16, 16, 32, 32, 96, 96, 256))))

    def to_c(self) -> _lib.NetConfigC:
        c = _lib.NetConfigC()
        c.in_channels, c.out_channels, c.hint_channels = self.in_channels, self.out_channels, self.hint_channels
        c.model_channels, c.num_res_blocks = self.model_channels, self.num_res_blocks
        c.n_levels = len(self.channel_mult)
        for i, m in enumerate(self.channel_mult):
            c.channel_mult[i] = m
        c.n_attention_resolutions = len(self.attention_resolutions)
        for i, a in enumerate(self.attention_resolutions):
            c.attention_resolutions[i] = a
        c.num_heads, c.transformer_depth, c.context_dim = self.num_heads, self.transformer_depth, self.context_dim
        for i, hw in enumerate(self.hint_widths):
            c.hint_widths[i] = hw
        return c

    @property
    def n_control(self) -> int:
        n = 1
        for level in range(len(self.channel_mult)):
            n += self.num_res_blocks + (1 if level != len(self.channel_mult) - 1 else 0)
        return n + 1


@dataclass
class VaeConfig:
    """first_stage_config.params.ddconfig of diffmodels/base_diffusion_makeup.yaml:86-107 (decoder half)."""
    z_channels: int = 4
    embed_dim: int = 4
    ch: int = 128
    ch_mult: Sequence[int] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    out_ch: int = 3

    @classmethod
    def from_yaml_params(cls, first_stage_params: dict) -> 'VaeConfig':
        dd = first_stage_params.get('ddconfig', first_stage_params)
        if dd.get('attn_resolutions'):
            raise NotImplementedError('decoder attention resolutions other than the mid block are not supported')
        return cls(z_channels=dd.get('z_channels', 4), embed_dim=first_stage_params.get('embed_dim', 4), ch=dd.get('ch', 128),
                   ch_mult=tuple(dd.get('ch_mult', (1, 2, 4, 4))), num_res_blocks=dd.get('num_res_blocks', 2),
                   out_ch=dd.get('out_ch', 3))

    def to_c(self) -> _lib.VaeConfigC:
        c = _lib.VaeConfigC()
        c.z_channels, c.embed_dim, c.ch, c.n_levels = self.z_channels, self.embed_dim, self.ch, len(self.ch_mult)
        for i, m in enumerate(self.ch_mult):
            c.ch_mult[i] = m
        c.num_res_blocks, c.out_ch = self.num_res_blocks, self.out_ch
        return c


@dataclass
class ClipConfig:
    """cond_stage_config FrozenCLIPEmbedder (diffmodels/base_diffusion_makeup.yaml:109-110): UPSTREAM default
    openai/clip-vit-large-patch14 text tower (vocab 49408, 77 positions, width 768, 12 layers x 12 heads, MLP 3072, quick-GELU)."""
    vocab_size: int = 49408
    max_positions: int = 77
    width: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    ln_eps: float = 1e-5

    @classmethod
    def from_yaml_params(cls, cond_stage_params: Optional[dict]) -> 'ClipConfig':
        p = dict(cond_stage_params or {})
        known = {k: p[k] for k in ('vocab_size', 'max_positions', 'width', 'layers', 'heads', 'intermediate', 'ln_eps') if k in p}
        if 'max_length' in p:
            known['max_positions'] = int(p['max_length'])
        return cls(**known)

    def to_c(self) -> _lib.ClipConfigC:
        c = _lib.ClipConfigC()
        c.vocab_size, c.max_positions, c.width, c.layers = self.vocab_size, self.max_positions, self.width, self.layers
        c.heads, c.intermediate, c.ln_eps = self.heads, self.intermediate, self.ln_eps
        return c


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def dpmpp_table(alphas: Sequence[float], alphas_prev: Sequence[float], order: int = 2,
                lower_order_final: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Coefficients of the multistep DPM-Solver++ on a DDIM step grid (include/mkd.h mkd_dpmpp_table; host only, needs no device):
    ``(coef [n, 6] float32, step_order [n] int32)``, row i = 1/alpha_t, sigma_t, c_x, c_0, c_1, c_2 of table entry i."""
    n = len(alphas)
    if n <= 0 or len(alphas_prev) != n:
        raise ValueError('alphas / alphas_prev must be non-empty and equally long')
    a = (C.c_float * n)(*[float(v) for v in alphas])
    ap = (C.c_float * n)(*[float(v) for v in alphas_prev])
    out = (C.c_float * (6 * n))()
    so = (C.c_int * n)()
    _lib.check(_lib.load().mkd_dpmpp_table(n, a, ap, int(order), int(bool(lower_order_final)), out, so), 'mkd_dpmpp_table')
    return np.ctypeslib.as_array(out).reshape(n, 6).copy(), np.ctypeslib.as_array(so).astype(np.int32)


def unipc_table(alphas: Sequence[float], alphas_prev: Sequence[float], order: int = 2, lower_order_final: bool = True,
                corrector: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Rows of the UniPC predictor-corrector on a DDIM step grid (include/mkd.h mkd_unipc_table; host only, needs no device):
    ``(coef [n, 12] float32, step_order [n] int32)``, row i = 1/alpha, sigma, a_c, q_0 .. q_3, a_p, p_0 .. p_2, 0 of table entry i."""
    n = len(alphas)
    if n <= 0 or len(alphas_prev) != n:
        raise ValueError('alphas / alphas_prev must be non-empty and equally long')
    a = (C.c_float * n)(*[float(v) for v in alphas])
    ap = (C.c_float * n)(*[float(v) for v in alphas_prev])
    out = (C.c_float * (12 * n))()
    so = (C.c_int * n)()
    lib = _lib.load()
    rc = lib.mkd_unipc_table(n, a, ap, int(order), int(bool(lower_order_final)), int(bool(corrector)), out, so)
    if rc == -1:          # MKD_ERR_ARG: a table this solver refuses
        msg = lib.mkd_last_error()
        raise ValueError(msg.decode() if msg else 'mkd_unipc_table: bad arguments')
    _lib.check(rc, 'mkd_unipc_table')
    return np.ctypeslib.as_array(out).reshape(n, 12).copy(), np.ctypeslib.as_array(so).astype(np.int32)


SOLVERS = {s.name: s.rows_id for s in _SOLVER.values() if s.rows_id is not None}          # the ids mkd_sample_rows takes
# numpy view of mkd_step_row (include/mkd.h), 64 bytes
STEP_ROW_DTYPE = np.dtype([('t', '<i8'), ('coef', '<f4', (4,)), ('sigma', '<f4'), ('dpm', '<f4', (6,)), ('temb_row', '<i4'),
                           ('active', '<i4'), ('scale', '<f4')])
assert STEP_ROW_DTYPE.itemsize == C.sizeof(_lib.StepRowC) == 64


def _solver_id(solver) -> int:
    if solver not in SOLVERS:
        raise ValueError(f"solver must be 'ddim' or 'dpmpp', got {solver!r}")
    return SOLVERS[solver]


def _row_field(row, name, default=None):
    return row.get(name, default) if isinstance(row, dict) else getattr(row, name, default)


def pack_sample_rows(rows, solver: str = 'ddim'):
    """``rows``: one request per sample, each an object (or dict) with ``timesteps`` and ``cfg_scale`` (default 1), for 'ddim'
    ``alphas`` / ``alphas_prev`` / ``sqrt_one_minus_alphas`` and optionally ``sigmas``, for 'dpmpp' ``dpm`` (the [n, 6] rows of
    ``dpmpp_table``); batching.build_rows makes them.  Returns (mkd_sample_row array, the host arrays it points at).  A table that is
    None stays a NULL pointer and a wrong length is the caller's error here (ValueError); everything else is checked by libmkd."""
    _solver_id(solver)
    rows = list(rows)
    if not rows:
        raise ValueError('rows must hold one request per sample')
    arr = (_lib.SampleRowC * len(rows))()
    keep = []
    for b, row in enumerate(rows):
        ts = _row_field(row, 'timesteps')
        n = 0 if ts is None else len(ts)
        arr[b].n_steps = n
        arr[b].cfg_scale = float(_row_field(row, 'cfg_scale', 1.0))
        if ts is not None:
            a = (C.c_int64 * max(n, 1))(*[int(v) for v in ts]); keep.append(a)
            arr[b].timesteps = C.cast(a, C.POINTER(C.c_int64))
        for name in ('alphas', 'alphas_prev', 'sqrt_one_minus_alphas', 'sigmas', 'dpm'):
            v = _row_field(row, name)
            if v is None:
                continue
            flat = np.asarray(v, dtype=np.float32).reshape(-1)
            if ts is not None and flat.size != (6 * n if name == 'dpm' else n):
                raise ValueError(f'rows[{b}].{name} has {flat.size} entries for {n} steps')
            a = (C.c_float * max(flat.size, 1))(*flat.tolist()); keep.append(a)
            setattr(arr[b], name, C.cast(a, C.POINTER(C.c_float)))
        n_over = _row_field(row, 'n_steps')          # (tests: a count that disagrees with the tables, e.g. 0 or beyond the limit)
        if n_over is not None:
            arr[b].n_steps = int(n_over)
    return arr, keep


def step_table(rows, solver: str = 'ddim') -> Tuple[np.ndarray, List[int]]:
    """The step table of a per-sample call (include/mkd.h mkd_step_table; host only, needs no device): ``(entries [S_max, B] of
    STEP_ROW_DTYPE, the call's distinct timesteps in first-seen order)``.  Executed step k, sample b: active while k < n_steps_b, table
    entry n_steps_b - 1 - k; a finished sample keeps the timestep / table row of its entry 0."""
    arr, keep = pack_sample_rows(rows, solver)
    lib = _lib.load()
    sm, nd = C.c_int(), C.c_int()
    _lib.check(lib.mkd_step_table(arr, len(arr), _solver_id(solver), None, C.byref(sm), None, C.byref(nd)), 'mkd_step_table')
    out = np.zeros((sm.value, len(arr)), dtype=STEP_ROW_DTYPE)
    ts = (C.c_int64 * max(nd.value, 1))()
    _lib.check(lib.mkd_step_table(arr, len(arr), _solver_id(solver), out.ctypes.data_as(C.POINTER(_lib.StepRowC)), None, ts, None),
               'mkd_step_table')
    del keep
    return out, [int(v) for v in ts[:nd.value]]


def sample_log_rows(n_steps: int, log_every_t: int) -> int:
    """Rows the in-library loop's trace keeps (include/mkd.h mkd_sample_log_rows; host only): the table entries i of an n_steps loop
    with ``i % log_every_t == 0 or i == n_steps - 1``."""
    rows = _lib.load().mkd_sample_log_rows(int(n_steps), int(log_every_t))
    if rows < 0:
        raise ValueError('sample_log_rows: n_steps >= 1 and log_every_t >= 1')
    return rows


def check_guidance_rescale(phi) -> float:
    """phi of the guidance rescale as a float in [0, 1] (ValueError otherwise)"""
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f'guidance_rescale must lie in [0, 1], got {phi}')
    return phi


class MkdEngine:
    """Owns one mkd_ctx on the current CUDA(HIP) device."""

    dpmpp_table = staticmethod(dpmpp_table)
    unipc_table = staticmethod(unipc_table)

    UNET_PREFIX = 'model.diffusion_model.'
    CONTROL_PREFIX = 'control_model.'

    def __init__(self, cfg: NetConfig, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise _lib.MkdError('MkdEngine needs a HIP device: the hot path has no CPU implementation')
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_ctx_create(C.byref(cfg.to_c()), C.byref(self._ctx)), 'mkd_ctx_create')
        self._keep: list = []          # tensors the prepared plan points at
        self.vae_cfg: Optional[VaeConfig] = None
        self.vae_enc_cfg: Optional[VaeConfig] = None
        self.clip_cfg: Optional[ClipConfig] = None
        self._prepared_key = None
        self.batch = 0
        self.latent_hw: Tuple[int, int] = (0, 0)

    def close(self):
        if self._ctx:
            self.lib.mkd_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ---------------------------------------------------------------------------------
    def expected_params(self) -> Dict[str, Tuple[int, ...]]:
        n = self.lib.mkd_param_total(self._ctx)
        out = {}
        shp = (C.c_int64 * 4)()
        for i in range(n):
            name = self.lib.mkd_param_name(self._ctx, i).decode()
            nd = self.lib.mkd_param_shape(self._ctx, i, shp)
            out[name] = tuple(int(shp[j]) for j in range(nd))
        return out

    def param_count(self, which: str) -> int:
        return int(self.lib.mkd_param_count(self._ctx, 0 if which == 'unet' else 4 if which == 'vae_encoder' else 1))

    def load_weight(self, name: str, tensor: torch.Tensor) -> None:
        t = tensor.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
        with torch.cuda.device(self.device):
            if t.is_cuda:
                torch.cuda.current_stream().synchronize()
            _lib.check(self.lib.mkd_load_weight(self._ctx, name.encode(), C.c_void_p(t.data_ptr()), t.dim(), shape),
                       f'mkd_load_weight({name})')

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> List[str]:
        """Loads every key under model.diffusion_model. / control_model. (upstream names); other keys
        (first_stage_model.*, cond_stage_model.*, teacher_model*) are returned as 'unused'."""
        expected = self.expected_params()
        unused = []
        for k, v in sd.items():
            if k in expected:
                self.load_weight(k, v)
            else:
                unused.append(k)
        missing = [k for k in expected if k not in sd]
        core_missing = [k for k in missing if not k.startswith(('first_stage_model.', 'cond_stage_model.'))]
        if core_missing and strict:
            raise _lib.MkdError(f'{len(core_missing)} weights missing from state_dict, e.g. {core_missing[:3]}')
        if not core_missing:
            self.finalize()
        enc = [k for k in missing if k.startswith(self.VAE_ENCODER_PREFIXES)]
        if getattr(self, 'vae_cfg', None) is not None and not [k for k in missing if k.startswith('first_stage_model.') and k not in enc]:
            self.finalize_vae()
        if getattr(self, 'vae_enc_cfg', None) is not None and not enc:
            self.finalize_vae_encoder()
        if getattr(self, 'clip_cfg', None) is not None and not [k for k in missing if k.startswith('cond_stage_model.')]:
            self.finalize_clip()
        return unused

    def init_random(self, seed: int = 0, gain: float = 1.0, norm_jitter: float = 0.0) -> None:
        """Seeded synthetic weights generated ON the device (bench / property tests): N(0, 1/fan_in) for
        every matrix/conv including upstream's zero-initialised ones, small biases, norm gamma = 1 + norm_jitter * N(0,1) and
        beta = norm_jitter * N(0,1) (0: the upstream initial values gamma 1 / beta 0)."""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for name, shape in self.expected_params().items():
            is_norm = ('.norm' in name or 'layer_norm' in name or 'in_layers.0' in name or 'out_layers.0' in name
                       or name.endswith('out.0.weight') or name.endswith('out.0.bias'))
            if len(shape) == 1:
                if is_norm:
                    t = (torch.ones if name.endswith('weight') else torch.zeros)(shape, device=self.device)
                    if norm_jitter:
                        t = t + norm_jitter * torch.randn(shape, generator=g, device=self.device)
                else:
                    t = 0.02 * torch.randn(shape, generator=g, device=self.device)
            else:
                fan_in = int(np.prod(shape[1:]))
                t = (gain / fan_in ** 0.5) * torch.randn(shape, generator=g, device=self.device)
            self.load_weight(name, t)
        self.finalize()

    def finalize(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_weights_finalize(self._ctx), 'mkd_weights_finalize')

    # ---- first-stage decoder -------------------------------------------------------------------------
    def configure_vae(self, vcfg: VaeConfig) -> None:
        """Adds the first_stage_model.{post_quant_conv,decoder}.* entries to expected_params(); load them like the rest."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_vae_configure(self._ctx, C.byref(vcfg.to_c())), 'mkd_vae_configure')
        self.vae_cfg = vcfg

    def finalize_vae(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_vae_finalize(self._ctx), 'mkd_vae_finalize')

    def decode(self, z: torch.Tensor, scale_factor: float = 0.18215) -> torch.Tensor:
        """decode_first_stage: z [B,4,h,w] -> images [B,3,8h,8w] fp32 (unclamped)."""
        z = _f32c(z, self.device)
        B, _, h, w = z.shape
        up = 2 ** (len(self.vae_cfg.ch_mult) - 1)
        out = torch.empty((B, self.vae_cfg.out_ch, h * up, w * up), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_decode(self._ctx, C.c_void_p(z.data_ptr()), B, h, w, float(scale_factor),
                                           C.c_void_p(out.data_ptr()), C.c_void_p(_stream())), 'mkd_decode')
        return out

    # ---- first-stage encoder (opt-in) ---------------------------------------------------------------------
    VAE_ENCODER_PREFIXES = ('first_stage_model.encoder.', 'first_stage_model.quant_conv.')

    def configure_vae_encoder(self, vcfg: VaeConfig) -> None:
        """Adds the first_stage_model.{encoder,quant_conv}.* entries to expected_params(); load them like the rest."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_vae_encoder_configure(self._ctx, C.byref(vcfg.to_c())), 'mkd_vae_encoder_configure')
        self.vae_enc_cfg = vcfg

    def finalize_vae_encoder(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_vae_encoder_finalize(self._ctx), 'mkd_vae_encoder_finalize')

    def encode(self, images: torch.Tensor, scale_factor: float = 0.18215, noise: Optional[torch.Tensor] = None,
               moments: bool = False):
        """get_first_stage_encoding(encode_first_stage(images)): images [B,3,H,W] -> z [B,4,H/f,W/f] fp32 (f = 2^(levels-1)).
        noise [B,4,H/f,W/f]: posterior sample() = mean + std * noise, None: mode().  moments=True: returns (z, moments
        [B,8,H/f,W/f]), the posterior's parameters before scaling."""
        if self.vae_enc_cfg is None:
            raise _lib.MkdError('encode: the first-stage encoder is not configured (configure_vae_encoder)')
        x = _f32c(images, self.device)
        B, _, H, W = x.shape
        f = 2 ** (len(self.vae_enc_cfg.ch_mult) - 1)
        zc = self.vae_enc_cfg.z_channels
        z = torch.empty((B, zc, H // f, W // f), device=self.device, dtype=torch.float32)
        mom = torch.empty((B, 2 * zc, H // f, W // f), device=self.device, dtype=torch.float32) if moments else None
        nz = _f32c(noise, self.device) if noise is not None else None
        if nz is not None and tuple(nz.shape) != tuple(z.shape):
            raise ValueError(f'encode: noise shape {tuple(nz.shape)} != latent shape {tuple(z.shape)}')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_encode(self._ctx, C.c_void_p(x.data_ptr()), B, H, W, float(scale_factor),
                                           C.c_void_p(_ptr(nz)), C.c_void_p(z.data_ptr()), C.c_void_p(_ptr(mom)),
                                           C.c_void_p(_stream())), 'mkd_encode')
        return (z, mom) if moments else z

    def encode_flops(self) -> float:
        return float(self.lib.mkd_encode_flops(self._ctx))

    # ---- CLIP text encoder ----------------------------------------------------------------------------
    CLIP_PREFIX = 'cond_stage_model.transformer.text_model.'

    def configure_clip(self, ccfg: ClipConfig) -> None:
        """Adds the cond_stage_model.transformer.text_model.* entries to expected_params(); load them like the rest."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_clip_configure(self._ctx, C.byref(ccfg.to_c())), 'mkd_clip_configure')
        self.clip_cfg = ccfg

    def finalize_clip(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_clip_finalize(self._ctx), 'mkd_clip_finalize')

    def encode_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """FrozenCLIPEmbedder.forward after tokenisation: ids [B, T<=77] -> last_hidden_state [B, T, width] fp32."""
        if getattr(self, 'clip_cfg', None) is None:
            raise _lib.MkdError('text encoder not configured (configure_clip)')
        if tokens.dim() != 2 or tokens.dtype not in (torch.int32, torch.int64):
            raise ValueError('tokens must be an integer [B, T] tensor')
        if tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= self.clip_cfg.vocab_size):
            raise ValueError(f'token id outside [0, {self.clip_cfg.vocab_size})')      # torch.nn.Embedding raises here too
        tok = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        B, T = tok.shape
        out = torch.empty((B, T, self.clip_cfg.width), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_clip_encode(self._ctx, C.c_void_p(tok.data_ptr()), B, T, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(_stream())), 'mkd_clip_encode')
        return out

    def set_option(self, name: str, value: float) -> None:
        """Per-context plan switch (include/mkd.h: mkd_ctx_set_option); takes effect at the next prepare()."""
        _lib.check(self.lib.mkd_ctx_set_option(self._ctx, name.encode(), float(value)), f'mkd_ctx_set_option({name})')

    def get_option(self, name: str) -> float:
        v = C.c_double()
        _lib.check(self.lib.mkd_ctx_get_option(self._ctx, name.encode(), C.byref(v)), f'mkd_ctx_get_option({name})')
        return v.value

    def debug_poison(self) -> None:
        """Tests only: NaN-fill everything one eps evaluation produces (see mkd_debug_poison)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_debug_poison(self._ctx), 'mkd_debug_poison')

    def decode_flops(self) -> float:
        return float(self.lib.mkd_decode_flops(self._ctx))

    # ---- conditioning / eval -----------------------------------------------------------------------
    def prepare(self, hint: Optional[torch.Tensor], context: torch.Tensor, latent_hw: Optional[Tuple[int, int]] = None,
                control_scales: Optional[Sequence[float]] = None, only_mid_control: bool = False,
                hint2: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None) -> None:
        """hint [B,6,8h,8w] in [0,1] or None (c_concat is None); context [B,77,ctx_dim]."""
        B = context.shape[0]
        ctx = _f32c(context, self.device)
        if ctx.shape[1] != 77 or ctx.shape[2] != self.cfg.context_dim:
            raise ValueError(f'context must be [B,77,{self.cfg.context_dim}], got {tuple(ctx.shape)}')
        hint_t = None
        if hint is not None:
            hint_t = _f32c(hint, self.device)
            if hint_t.shape[0] != B or hint_t.shape[1] != self.cfg.hint_channels or hint_t.shape[2] % 8 or hint_t.shape[3] % 8:
                raise ValueError(f'hint must be [B,{self.cfg.hint_channels},8h,8w], got {tuple(hint_t.shape)}')
            h, w = hint_t.shape[2] // 8, hint_t.shape[3] // 8
            if latent_hw is not None and tuple(latent_hw) != (h, w):
                raise ValueError('latent_hw disagrees with the hint size')
        else:
            if latent_hw is None:
                raise ValueError('latent_hw is required when hint is None')
            h, w = latent_hw
        scales = None
        if control_scales is not None:
            if len(control_scales) != self.cfg.n_control:
                raise ValueError(f'control_scales must have {self.cfg.n_control} entries')
            scales = (C.c_float * len(control_scales))(*[float(s) for s in control_scales])
        hint2_t = alpha_t = None
        if hint2 is not None:
            if hint_t is None or alpha is None:
                raise ValueError('interpolation needs hint, hint2 and alpha')
            hint2_t = _f32c(hint2, self.device)
            alpha_t = _f32c(alpha, self.device).reshape(-1)
            if tuple(hint2_t.shape) != tuple(hint_t.shape) or alpha_t.shape[0] != B:
                raise ValueError('hint2 must match hint and alpha must have one entry per sample')
        with torch.cuda.device(self.device):
            if hint2_t is None:
                _lib.check(self.lib.mkd_prepare(self._ctx, B, h, w, C.c_void_p(_ptr(hint_t)), C.c_void_p(ctx.data_ptr()),
                                                scales, int(bool(only_mid_control)), C.c_void_p(_stream())), 'mkd_prepare')
            else:
                _lib.check(self.lib.mkd_prepare_interp(self._ctx, B, h, w, C.c_void_p(hint_t.data_ptr()), C.c_void_p(hint2_t.data_ptr()),
                                                       C.c_void_p(alpha_t.data_ptr()), C.c_void_p(ctx.data_ptr()), scales,
                                                       int(bool(only_mid_control)), C.c_void_p(_stream())), 'mkd_prepare_interp')
        self._keep = [hint_t, ctx, hint2_t, alpha_t]
        self.batch, self.latent_hw = B, (h, w)

    def prepare_regions(self, hints: Sequence[torch.Tensor], weights: torch.Tensor, context: torch.Tensor,
                        control_scales: Optional[Sequence[float]] = None, only_mid_control: bool = False) -> None:
        """Region-wise transfer from several references (include/mkd.h mkd_prepare_regions): ``hints`` R <= 8 tensors
        [B,6,8h,8w] (src || ref_r, index 0 the base), ``weights`` fp32 [B,R,h,w]; the ControlNet sees sum_r weights[:, r] * E(hints[r])."""
        hints = list(hints)
        R = len(hints)
        if not 1 <= R <= 8:
            raise ValueError(f'prepare_regions takes 1..8 hints, got {R}')
        B = context.shape[0]
        ctx = _f32c(context, self.device)
        if ctx.dim() != 3 or ctx.shape[1] != 77 or ctx.shape[2] != self.cfg.context_dim:
            raise ValueError(f'context must be [B,77,{self.cfg.context_dim}], got {tuple(ctx.shape)}')
        hs = [_f32c(t, self.device) for t in hints]
        shp = tuple(hs[0].shape)
        if len(shp) != 4 or shp[0] != B or shp[1] != self.cfg.hint_channels or shp[2] % 8 or shp[3] % 8 or any(tuple(t.shape) != shp for t in hs):
            raise ValueError(f'every hint must be [B,{self.cfg.hint_channels},8h,8w] with equal shapes, got {[tuple(t.shape) for t in hs]}')
        h, w = shp[2] // 8, shp[3] // 8
        wt = _f32c(weights, self.device)
        if tuple(wt.shape) != (B, R, h, w):
            raise ValueError(f'weights must be [{B},{R},{h},{w}], got {tuple(wt.shape)}')
        scales = None
        if control_scales is not None:
            if len(control_scales) != self.cfg.n_control:
                raise ValueError(f'control_scales must have {self.cfg.n_control} entries')
            scales = (C.c_float * len(control_scales))(*[float(s) for s in control_scales])
        ptrs = (C.c_void_p * R)(*[t.data_ptr() for t in hs])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_prepare_regions(self._ctx, B, h, w, ptrs, R, C.c_void_p(wt.data_ptr()), C.c_void_p(ctx.data_ptr()),
                                                    scales, int(bool(only_mid_control)), C.c_void_p(_stream())), 'mkd_prepare_regions')
        self._keep = [hs, ctx, wt]
        self.batch, self.latent_hw = B, (h, w)

    def region_weights(self, masks: torch.Tensor, factor: int = 8, feather: int = 1, strength: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Region masks uint8 [K,B,H,W] (K = 1..7; a pixel belongs to the lowest k whose mask is non-zero) -> blend weights fp32
        [B,K+1,H/factor,W/factor] on the device (include/mkd.h mkd_region_weights): plane k+1 = strength[b,k] x the owned fraction of the
        (2 feather + 1)^2 block window, plane 0 = what is left of 1.  ``strength`` [B,K] or None (all ones)."""
        if masks.dim() != 4 or masks.dtype != torch.uint8:
            raise ValueError(f'masks must be uint8 [K,B,H,W], got {masks.dtype} {tuple(masks.shape)}')
        K, B, H, W = masks.shape
        if not 1 <= K <= 7:
            raise ValueError(f'1..7 region masks, got {K}')
        if not 1 <= int(factor) <= 64 or H % int(factor) or W % int(factor):
            raise ValueError(f'masks {H}x{W} are not a multiple of factor {factor} (1..64)')
        if not 0 <= int(feather) <= 4:
            raise ValueError(f'feather must be 0..4 latent pixels, got {feather}')
        m = masks.to(self.device).contiguous()
        st = None
        if strength is not None:
            st = _f32c(strength, self.device)
            if tuple(st.shape) != (B, K):
                raise ValueError(f'strength must be [{B},{K}], got {tuple(st.shape)}')
        out = torch.empty((B, K + 1, H // int(factor), W // int(factor)), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_region_weights(C.c_void_p(m.data_ptr()), K, B, H, W, int(factor), int(feather), C.c_void_p(_ptr(st)),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(_stream())), 'mkd_region_weights')
        return out

    def debug_hint_embedding(self) -> torch.Tensor:
        """Tests only: the cached ControlNet hint embedding [B,h,w,model_channels] bf16 (see mkd_debug_hint_embedding)."""
        out = torch.empty((self.batch, *self.latent_hw, self.cfg.model_channels), device=self.device, dtype=torch.bfloat16)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_debug_hint_embedding(self._ctx, C.c_void_p(out.data_ptr()), C.c_void_p(_stream())),
                       'mkd_debug_hint_embedding')
        return out

    def eps(self, x: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One apply_model evaluation on the prepared conditioning. x [B,4,h,w] fp32, t [B] int64."""
        x = _f32c(x, self.device)
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(x.shape) != (self.batch, self.cfg.in_channels, *self.latent_hw) or t.shape[0] != self.batch:
            raise ValueError(f'x/t do not match the prepared batch {self.batch} x {self.latent_hw}: {tuple(x.shape)}')
        if out is None:
            out = torch.empty((self.batch, self.cfg.out_channels, *self.latent_hw), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_eps(self._ctx, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream())), 'mkd_eps')
        return out

    def cfg_rescale_factor(self, eps_c: torch.Tensor, eps_u: torch.Tensor, cfg_scale: float, phi: float) -> torch.Tensor:
        """Guidance-rescale factors (mkd_cfg_rescale_factor): k [B] = phi std(eps_c[b]) / std(g[b]) + (1 - phi) per sample of
        [B, ...] tensors, g = eps_u + cfg_scale (eps_c - eps_u)."""
        phi = check_guidance_rescale(phi)
        eps_c = _f32c(eps_c, self.device); eps_u = _f32c(eps_u, self.device)
        if eps_c.dim() < 2 or eps_u.shape != eps_c.shape:
            raise ValueError('cfg_rescale_factor: eps_c and eps_u must be [B, ...] tensors of one shape')
        k = torch.empty(eps_c.shape[0], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_cfg_rescale_factor(C.c_void_p(eps_c.data_ptr()), C.c_void_p(eps_u.data_ptr()), float(cfg_scale), phi,
                                                       eps_c.shape[0], eps_c[0].numel(), C.c_void_p(k.data_ptr()), C.c_void_p(_stream())),
                       'mkd_cfg_rescale_factor')
        return k

    def _rescale_k(self, eps_c, eps_u, cfg_scale, guidance_rescale):
        """(k [B] or None, elements per sample) of one stand-alone step: engaged only with an unconditional half and phi > 0"""
        phi = check_guidance_rescale(guidance_rescale)
        if eps_u is None or phi == 0.0:
            return None, 0
        return self.cfg_rescale_factor(eps_c, eps_u, cfg_scale, phi), eps_c[0].numel()

    def ddim_step(self, x, eps_c, eps_u, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, noise=None,
                  temperature: float = 1.0, want_x0: bool = True, guidance_rescale: float = 0.0):
        x = _f32c(x, self.device); eps_c = _f32c(eps_c, self.device)
        eps_u = None if eps_u is None else _f32c(eps_u, self.device)
        noise = None if noise is None else _f32c(noise, self.device)
        x_prev = torch.empty_like(x)
        x0 = torch.empty_like(x) if want_x0 else None
        self._step_call(_SOLVER['ddim'], (C.c_void_p(x.data_ptr()), C.c_void_p(eps_c.data_ptr()), C.c_void_p(_ptr(eps_u)), float(cfg_scale),
                                      float(a_t), float(a_prev), float(sigma_t), float(sqrt_one_minus_at), C.c_void_p(_ptr(noise)),
                                      float(temperature)), (C.c_void_p(x_prev.data_ptr()), C.c_void_p(_ptr(x0)), x.numel()),
                        eps_c, eps_u, cfg_scale, guidance_rescale)
        return x_prev, x0

    def _step_call(self, solver, head, tail, eps_c, eps_u, cfg_scale, guidance_rescale):
        """One stand-alone step kernel of ``solver`` (its sampling.Solver record): mkd_<step>(*head, *tail, stream); with the guidance
        rescale engaged the factor launch, then mkd_<step>_ex with (k, n_per_sample) between head and tail (the in-library loop's two
        kernels)."""
        entry = 'mkd_' + solver.step
        k, per = self._rescale_k(eps_c, eps_u, cfg_scale, guidance_rescale)
        if k is not None:
            entry, head = entry + '_ex', (*head, C.c_void_p(k.data_ptr()), per)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, entry)(*head, *tail, C.c_void_p(_stream())), entry)

    def sample(self, x_T: torch.Tensor, timesteps: Sequence[int], alphas: Sequence[float], alphas_prev: Sequence[float],
               sqrt_one_minus_alphas: Sequence[float], cfg_scale: float = 1.0, use_graph: bool = False,
               sigmas: Optional[Sequence[float]] = None, noise: Optional[torch.Tensor] = None, temperature: float = 1.0,
               x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, q_sqrt_ac: Optional[Sequence[float]] = None,
               q_sqrt_1m_ac: Optional[Sequence[float]] = None, q_noise: Optional[torch.Tensor] = None,
               log_every_t: int = 100, want_trace: bool = False, guidance_rescale: float = 0.0):
        """Whole reverse loop in one call (cddim.py:81-100). Prepared batch must be B or 2B (CFG).  eta > 0 (cddim.py:74-78):
        ``sigmas`` like the other tables and ``noise`` [n_steps, B, 4, h, w], row k = the draw of the k-th executed step.
        Masked sampling (include/mkd.h mkd_sample_masked): ``x0`` [B,4,h,w], ``mask`` [1|B, 1|4, h, w] (1 keeps x0), the DDPM
        tables at each entry's timestep ``q_sqrt_ac`` / ``q_sqrt_1m_ac`` (indexed like ``alphas``) and ``q_noise`` [n_steps, B, 4, h, w].
        ``want_trace``: returns ``(latent, x_inter, pred_x0)``, the two [rows, B, 4, h, w] tensors of the sampler's intermediates
        logged by ``log_every_t`` (mkd_sample_extras); ``guidance_rescale`` = phi in [0, 1], engaged with guidance and phi > 0."""
        return self._sample_call(_SOLVER['ddim'], x_T, timesteps,
                                 dict(alphas=alphas, alphas_prev=alphas_prev, sqrt_one_minus_alphas=sqrt_one_minus_alphas), (), cfg_scale, use_graph, (x0, mask, q_sqrt_ac, q_sqrt_1m_ac, q_noise), log_every_t, want_trace, guidance_rescale,
                                 eta=(sigmas, noise, temperature))

    def _sample_call(self, solver, x_T, timesteps, tables, args, cfg_scale, use_graph, masking, log_every_t, want_trace, guidance_rescale, eta=None):
        """The body of sample / sample_dpmpp / sample_unipc (``solver``: the sampling.Solver record).  The multistep solvers (eta None)
        call mkd_<loop>, or mkd_<loop>_ex with a trace or phi != 0, with ``args`` = their options after the tables; DDIM calls
        mkd_sample_masked_ex with either, else mkd_sample_masked with a mask, else mkd_sample_eta with a non-zero sigma, else mkd_sample."""
        x_T = self._check_x_T(x_T, cfg_scale)
        n, ts, tables = self._sample_tables(timesteps, **tables)
        out = torch.empty_like(x_T)
        qm, keep = self._sample_mask(x_T, n, *masking)
        ex, rows = self._sample_extras(x_T, n, log_every_t, want_trace, guidance_rescale)
        qm_ex = (None if qm is None else C.byref(qm), *(() if ex is None else (C.byref(ex),)))
        noise = None
        if eta is None:
            entry, args = 'mkd_' + solver.loop + ('_ex' if ex is not None else ''), (*args, *qm_ex)
        else:
            sigmas, noise, temperature = eta
            sg = None
            if sigmas is not None and any(float(v) != 0.0 for v in sigmas):
                if len(sigmas) != n:
                    raise ValueError('sigmas must be as long as timesteps')
                if noise is None or tuple(noise.shape) != (n, *x_T.shape):
                    raise ValueError(f'eta > 0 needs noise of shape {(n, *x_T.shape)} (one draw per executed step)')
                noise = _f32c(noise, self.device)
                sg = (C.c_float * n)(*[float(v) for v in sigmas])
            else:
                noise = None
            args = (sg, C.c_void_p(_ptr(noise)), float(temperature))
            if ex is not None:
                entry, args = 'mkd_sample_masked_ex', (*args, *qm_ex)
            elif qm is not None:
                entry, args = 'mkd_sample_masked', (*args, *qm_ex)
            elif sg is not None:
                entry = 'mkd_sample_eta'
            else:
                entry, args = 'mkd_sample', ()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, entry)(self._ctx, C.c_void_p(x_T.data_ptr()), x_T.shape[0], n, ts, *tables, *args, float(cfg_scale),
                                                C.c_void_p(out.data_ptr()), int(use_graph), C.c_void_p(_stream())), entry)
        if qm is not None:
            self._hold(keep, noise)
        elif noise is not None and use_graph:
            torch.cuda.synchronize(self.device)          # the replayed loop reads `noise` after this call returns: keep it alive
        return (out, *rows) if want_trace else out

    def _sample_extras(self, x_T, n, log_every_t, want_trace, guidance_rescale):
        """(mkd_sample_extras or None when neither feature is asked for: today's entry is called; the trace tensors or ()).  The rows
        are returned to the caller, whose stream waits for the loop: they outlive the enqueued work."""
        phi = check_guidance_rescale(guidance_rescale)
        if not want_trace and phi == 0.0:
            return None, ()
        rows = ()
        ex = _lib.SampleExtrasC(1, 0, None, None, phi)
        if want_trace:
            if int(log_every_t) < 1:
                raise ValueError(f'log_every_t must be >= 1, got {log_every_t}')
            r = sample_log_rows(n, int(log_every_t))
            rows = (torch.empty((r, *x_T.shape), device=self.device, dtype=torch.float32),
                    torch.empty((r, *x_T.shape), device=self.device, dtype=torch.float32))
            ex = _lib.SampleExtrasC(int(log_every_t), r, rows[0].data_ptr(), rows[1].data_ptr(), phi)
        return ex, rows

    def dpmpp_step(self, x, eps_c, eps_u, cfg_scale, coef6, m1=None, m2=None, guidance_rescale: float = 0.0):
        """One DPM-Solver++ multistep update (mkd_dpmpp_step): ``coef6`` = a row of ``dpmpp_table``; m1 / m2 = the x0-predictions
        of the previous two steps, needed where coef6[4] / coef6[5] is non-zero.  Returns (x_prev, m0)."""
        x = _f32c(x, self.device); eps_c = _f32c(eps_c, self.device)
        eps_u = None if eps_u is None else _f32c(eps_u, self.device)
        k = [float(np.float32(v)) for v in coef6]
        if len(k) != 6:
            raise ValueError('coef6 must have six entries (a row of dpmpp_table)')
        if (k[4] != 0.0 and m1 is None) or (k[5] != 0.0 and m2 is None):
            raise ValueError('dpmpp_step: a non-zero history coefficient needs its x0-prediction')
        m1 = None if (m1 is None or k[4] == 0.0) else _f32c(m1, self.device)
        m2 = None if (m2 is None or k[5] == 0.0) else _f32c(m2, self.device)
        for t in (eps_c, eps_u, m1, m2):
            if t is not None and t.numel() != x.numel():
                raise ValueError('dpmpp_step: every tensor must have the size of x')
        x_prev = torch.empty_like(x)
        m0 = torch.empty_like(x)
        self._step_call(_SOLVER['dpmpp'], (C.c_void_p(x.data_ptr()), C.c_void_p(eps_c.data_ptr()), C.c_void_p(_ptr(eps_u)), float(cfg_scale),
                                       (C.c_float * 6)(*k), C.c_void_p(_ptr(m1)), C.c_void_p(_ptr(m2))),
                        (C.c_void_p(x_prev.data_ptr()), C.c_void_p(m0.data_ptr()), x.numel()), eps_c, eps_u, cfg_scale, guidance_rescale)
        return x_prev, m0

    def sample_dpmpp(self, x_T: torch.Tensor, timesteps: Sequence[int], alphas: Sequence[float], alphas_prev: Sequence[float],
                     order: int = 2, lower_order_final: bool = True, cfg_scale: float = 1.0, use_graph: bool = False,
                     x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, q_sqrt_ac: Optional[Sequence[float]] = None,
                     q_sqrt_1m_ac: Optional[Sequence[float]] = None, q_noise: Optional[torch.Tensor] = None,
                     log_every_t: int = 100, want_trace: bool = False, guidance_rescale: float = 0.0):
        """The whole DPM-Solver++ multistep loop in one call (mkd_sample_dpmpp): ``sample``'s contract on the same DDIM tables
        (prepared batch B or 2B with guidance, masked sampling through x0 / mask / q_*), deterministic.  ``want_trace`` /
        ``log_every_t`` / ``guidance_rescale`` as in ``sample`` (the pred_x0 rows are the solver's m_k)."""
        return self._sample_call(_SOLVER['dpmpp'], x_T, timesteps, dict(alphas=alphas, alphas_prev=alphas_prev),
                                 (int(order), int(bool(lower_order_final))), cfg_scale, use_graph, (x0, mask, q_sqrt_ac, q_sqrt_1m_ac, q_noise),
                                 log_every_t, want_trace, guidance_rescale)

    def unipc_step(self, x, xc_prev, eps_c, eps_u, cfg_scale, coef12, m1=None, m2=None, m3=None, guidance_rescale: float = 0.0):
        """One UniPC step (mkd_unipc_step): ``x`` = the predicted latent the model was evaluated at, ``xc_prev`` = the previous corrected
        latent, ``coef12`` = a row of ``unipc_table``, m1 / m2 / m3 = the x0-predictions of the previous three steps; each is needed
        where a coefficient of its own is non-zero.  Returns (x_next, xc, m0): the next predicted latent, this step's corrected latent
        and x0-prediction."""
        x = _f32c(x, self.device); eps_c = _f32c(eps_c, self.device)
        eps_u = None if eps_u is None else _f32c(eps_u, self.device)
        k = [float(np.float32(v)) for v in coef12]
        if len(k) != 12:
            raise ValueError('coef12 must have twelve entries (a row of unipc_table)')
        cor = k[2] != 0.0
        need = (cor, (cor and k[4] != 0.0) or k[9] != 0.0, (cor and k[5] != 0.0) or k[10] != 0.0, cor and k[6] != 0.0)
        given = [xc_prev, m1, m2, m3]
        if any(nd and t is None for nd, t in zip(need, given)):
            raise ValueError('unipc_step: a non-zero coefficient needs its corrected latent / x0-prediction')
        xc_prev, m1, m2, m3 = (_f32c(t, self.device) if nd else None for nd, t in zip(need, given))
        for t in (eps_c, eps_u, xc_prev, m1, m2, m3):
            if t is not None and t.numel() != x.numel():
                raise ValueError('unipc_step: every tensor must have the size of x')
        x_next, xc, m0 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        self._step_call(_SOLVER['unipc'], (C.c_void_p(x.data_ptr()), C.c_void_p(_ptr(xc_prev)), C.c_void_p(eps_c.data_ptr()), C.c_void_p(_ptr(eps_u)),
                                       float(cfg_scale), (C.c_float * 12)(*k), C.c_void_p(_ptr(m1)), C.c_void_p(_ptr(m2)), C.c_void_p(_ptr(m3))),
                        (C.c_void_p(x_next.data_ptr()), C.c_void_p(xc.data_ptr()), C.c_void_p(m0.data_ptr()), x.numel()),
                        eps_c, eps_u, cfg_scale, guidance_rescale)
        return x_next, xc, m0

    def sample_unipc(self, x_T: torch.Tensor, timesteps: Sequence[int], alphas: Sequence[float], alphas_prev: Sequence[float],
                     order: int = 2, lower_order_final: bool = True, corrector: bool = True, cfg_scale: float = 1.0,
                     use_graph: bool = False, x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     q_sqrt_ac: Optional[Sequence[float]] = None, q_sqrt_1m_ac: Optional[Sequence[float]] = None,
                     q_noise: Optional[torch.Tensor] = None, log_every_t: int = 100, want_trace: bool = False,
                     guidance_rescale: float = 0.0):
        """The whole UniPC predictor-corrector loop in one call (mkd_sample_unipc): ``sample_dpmpp``'s contract on the same DDIM tables,
        which must be contiguous (alphas_prev[i] == alphas[i - 1]).  ``want_trace`` / ``log_every_t`` / ``guidance_rescale`` as in
        ``sample`` (x_inter rows: the predicted latents; pred_x0 rows: the solver's m_k).  Masked sampling (x0 / mask / q_*) is not
        defined for this solver: libmkd refuses it (MkdError, -4) and the context stays usable."""
        return self._sample_call(_SOLVER['unipc'], x_T, timesteps, dict(alphas=alphas, alphas_prev=alphas_prev),
                                 (int(order), int(bool(lower_order_final)), int(bool(corrector))), cfg_scale, use_graph,
                                 (x0, mask, q_sqrt_ac, q_sqrt_1m_ac, q_noise), log_every_t, want_trace, guidance_rescale)

    # ---- per-sample requests in one batch (include/mkd.h mkd_sample_rows) ------------------------------------------------------
    def sample_rows(self, x_T: torch.Tensor, rows, solver: str = 'ddim', noise: Optional[torch.Tensor] = None, temperature: float = 1.0,
                    use_graph: bool = False, x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                    want_trace: bool = False, guidance_rescale: float = 0.0) -> torch.Tensor:
        """The whole reverse loop with one request per sample: ``rows`` as for ``pack_sample_rows`` (batching.build_rows), each with its
        own schedule, guidance scale and sigmas.  All samples start together, short ones finish first and are not touched again.  The
        prepared batch is B when every scale is 1, else 2B (unconditional half first).  eta > 0: ``noise`` [S_max, B, 4, h, w], row k =
        the draw of executed step k.  Row b has the bits of the uniform call with sample b's request.  ``x0`` / ``mask`` /
        ``want_trace`` / ``guidance_rescale`` are not combined with per-sample rows: libmkd refuses them (MkdError)."""
        x_T = _f32c(x_T, self.device)
        rows = list(rows)
        arr, keep = pack_sample_rows(rows, solver)
        if x_T.dim() != 4 or tuple(x_T.shape[1:]) != (self.cfg.in_channels, *self.latent_hw) or x_T.shape[0] != len(arr):
            # libmkd copies batch * C * h * w floats using the PREPARED h, w: a smaller latent would be read out of bounds
            raise ValueError(f'x_T {tuple(x_T.shape)} does not match the rows / the prepared latent: expected '
                             f'({len(arr)}, {self.cfg.in_channels}, {self.latent_hw[0]}, {self.latent_hw[1]})')
        rows = list(rows)
        lens = [0 if _row_field(r, 'timesteps') is None else len(_row_field(r, 'timesteps')) for r in rows]
        s_max = max(lens)
        stochastic = solver == 'ddim' and any(_row_field(r, 'sigmas') is not None and any(float(v) != 0.0 for v in _row_field(r, 'sigmas'))
                                              for r in rows)
        if stochastic:
            if noise is None or tuple(noise.shape) != (s_max, *x_T.shape):
                raise ValueError(f'eta > 0 needs noise of shape {(s_max, *x_T.shape)} (one draw per executed step)')
            noise = _f32c(noise, self.device)
        else:
            noise = None
        qm = None
        if x0 is not None or mask is not None:
            qm = _lib.SampleMaskC(_ptr(x0), _ptr(mask), 1, 1, None, None, None)
        ex = None
        phi = check_guidance_rescale(guidance_rescale)
        if want_trace or phi != 0.0:
            dummy = torch.empty_like(x_T) if want_trace else None
            ex = _lib.SampleExtrasC(1, 1, _ptr(dummy), None, phi)
        out = torch.empty_like(x_T)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_sample_rows(self._ctx, C.c_void_p(x_T.data_ptr()), len(arr), arr, _solver_id(solver),
                                                C.c_void_p(_ptr(noise)), float(temperature), None if qm is None else C.byref(qm),
                                                None if ex is None else C.byref(ex), C.c_void_p(out.data_ptr()), int(use_graph),
                                                C.c_void_p(_stream())), 'mkd_sample_rows')
        # the replayed loop reads `noise` after this call returns: it stays referenced until the next per-sample call.  No host wait:
        # the caller's stream waits for the loop, so the caching allocator can only hand the block to work ordered after it
        self._rows_keep = noise
        del keep
        return out

    def _step_entries(self, entries, B: int) -> torch.Tensor:
        """[B] step-table entries (STEP_ROW_DTYPE array, or a uint8 device tensor [B, 64]) on the device"""
        if isinstance(entries, torch.Tensor):
            e = entries.to(self.device).contiguous()
        else:
            e = np.ascontiguousarray(np.asarray(entries, dtype=STEP_ROW_DTYPE).reshape(-1))
            e = torch.from_numpy(e.view(np.uint8).reshape(-1, STEP_ROW_DTYPE.itemsize).copy()).to(self.device)
        if e.dtype != torch.uint8 or tuple(e.shape) != (B, STEP_ROW_DTYPE.itemsize):
            raise ValueError(f'entries must be {B} step-table entries of {STEP_ROW_DTYPE.itemsize} bytes')
        return e

    @staticmethod
    def _same_numel(x, **named):
        for name, t in named.items():
            if t is not None and (t.numel() != x.numel() or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device):
                raise ValueError(f'{name} must be a contiguous fp32 tensor of the size of x on its device')

    def ddim_step_rows(self, x, eps_c, eps_u, entries, noise=None, temperature: float = 1.0, x_prev=None, pred_x0=None, want_x0: bool = True):
        """One per-sample DDIM update (mkd_ddim_step_rows): sample b of the [B, ...] tensors uses ``entries[b]`` (a row of
        ``step_table``); finished samples (active = 0) are not read and no byte of their ``x_prev`` / ``pred_x0`` rows is written
        (pass the tensors in to see that).  Returns (x_prev, pred_x0)."""
        x = _f32c(x, self.device); eps_c = _f32c(eps_c, self.device)
        eps_u = None if eps_u is None else _f32c(eps_u, self.device)
        noise = None if noise is None else _f32c(noise, self.device)
        B = x.shape[0]
        e = self._step_entries(entries, B)
        if x_prev is None:
            x_prev = torch.zeros_like(x)
        if pred_x0 is None and want_x0:
            pred_x0 = torch.zeros_like(x)
        self._same_numel(x, eps_c=eps_c, eps_u=eps_u, noise=noise, x_prev=x_prev, pred_x0=pred_x0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_ddim_step_rows(C.c_void_p(x.data_ptr()), C.c_void_p(eps_c.data_ptr()), C.c_void_p(_ptr(eps_u)),
                                                   C.c_void_p(e.data_ptr()), C.c_void_p(_ptr(noise)), float(temperature),
                                                   C.c_void_p(x_prev.data_ptr()), C.c_void_p(_ptr(pred_x0)), B, x[0].numel(),
                                                   C.c_void_p(_stream())), 'mkd_ddim_step_rows')
        return x_prev, pred_x0

    def dpmpp_step_rows(self, x, eps_c, eps_u, entries, m1, m2, x_prev=None, m0=None):
        """One per-sample DPM-Solver++ update (mkd_dpmpp_step_rows), as ``ddim_step_rows``: m1 / m2 = the previous two
        x0-predictions (read where the entry's c_1 / c_2 is non-zero).  Returns (x_prev, m0)."""
        x = _f32c(x, self.device); eps_c = _f32c(eps_c, self.device)
        eps_u = None if eps_u is None else _f32c(eps_u, self.device)
        m1 = _f32c(m1, self.device); m2 = _f32c(m2, self.device)
        B = x.shape[0]
        e = self._step_entries(entries, B)
        if x_prev is None:
            x_prev = torch.zeros_like(x)
        if m0 is None:
            m0 = torch.zeros_like(x)
        self._same_numel(x, eps_c=eps_c, eps_u=eps_u, m1=m1, m2=m2, x_prev=x_prev, m0=m0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_dpmpp_step_rows(C.c_void_p(x.data_ptr()), C.c_void_p(eps_c.data_ptr()), C.c_void_p(_ptr(eps_u)),
                                                    C.c_void_p(e.data_ptr()), C.c_void_p(m1.data_ptr()), C.c_void_p(m2.data_ptr()),
                                                    C.c_void_p(x_prev.data_ptr()), C.c_void_p(m0.data_ptr()), B, x[0].numel(),
                                                    C.c_void_p(_stream())), 'mkd_dpmpp_step_rows')
        return x_prev, m0

    def _check_x_T(self, x_T: torch.Tensor, cfg_scale: float) -> torch.Tensor:
        """x_T as the fp32 device tensor, checked against the prepared conditioning (batch B, or 2B = [uncond; cond] with guidance)."""
        x_T = _f32c(x_T, self.device)
        cfg_on = float(cfg_scale) != 1.0
        want_b = self.batch // 2 if cfg_on else self.batch
        if (x_T.dim() != 4 or tuple(x_T.shape[1:]) != (self.cfg.in_channels, *self.latent_hw) or x_T.shape[0] != want_b
                or (cfg_on and self.batch % 2)):
            # libmkd copies batch * C * h * w floats using the PREPARED h, w: a smaller latent would be read out of bounds
            raise ValueError(f'x_T {tuple(x_T.shape)} does not match the prepared conditioning: expected '
                             f'({want_b}, {self.cfg.in_channels}, {self.latent_hw[0]}, {self.latent_hw[1]})'
                             + (' (CFG: prepared batch is [uncond; cond])' if cfg_on else ''))
        return x_T

    @staticmethod
    def _sample_tables(timesteps, **tables):
        """(n, timesteps as c_int64[n], the named per-step tables as c_float[n] each); all must be non-empty and equally long."""
        n = len(timesteps)
        if n <= 0 or any(len(v) != n for v in tables.values()):
            raise ValueError(f'{" / ".join(["timesteps", *tables])} must be non-empty and equally long')
        return n, (C.c_int64 * n)(*[int(v) for v in timesteps]), [(C.c_float * n)(*[float(v) for v in t]) for t in tables.values()]

    def _hold(self, keep, noise) -> None:
        """A masked call's tensors / arrays stay referenced until the next masked call.  No host wait: the caller's stream waits for
        the replayed loop, so the caching allocator can only hand these blocks to work ordered after it."""
        if keep is not None:
            self._loop_keep = (keep, noise)

    def _mask_geometry(self, mask: torch.Tensor, B: int, Cn: int, hw) -> Tuple[int, int]:
        if mask.dim() != 4 or tuple(mask.shape[2:]) != tuple(hw) or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, Cn):
            raise ValueError(f'mask must be [1 or {B}, 1 or {Cn}, {hw[0]}, {hw[1]}], got {tuple(mask.shape)}')
        return int(mask.shape[0]), int(mask.shape[1])

    def _sample_mask(self, x_T, n, x0, mask, q_sqrt_ac, q_sqrt_1m_ac, q_noise):
        """Validated mkd_sample_mask for sample(); returns it with the tensors / arrays it points at ((None, None): no masking)."""
        if x0 is None and mask is None:
            return None, None
        if x0 is None or mask is None:
            raise ValueError('masked sampling needs both mask and x0')
        x0 = _f32c(x0, self.device)
        if tuple(x0.shape) != tuple(x_T.shape):
            raise ValueError(f'x0 must be [{", ".join(map(str, x_T.shape))}] (the un-doubled batch), got {tuple(x0.shape)}')
        mb, mc = self._mask_geometry(mask, x_T.shape[0], x_T.shape[1], x_T.shape[2:])
        mask = _f32c(mask, self.device)
        if q_sqrt_ac is None or q_sqrt_1m_ac is None or len(q_sqrt_ac) != n or len(q_sqrt_1m_ac) != n:
            raise ValueError('masked sampling needs q_sqrt_ac and q_sqrt_1m_ac as long as timesteps')
        if q_noise is None or tuple(q_noise.shape) != (n, *x_T.shape):
            raise ValueError(f'masked sampling needs q_noise of shape {(n, *x_T.shape)} (one draw per executed step)')
        q_noise = _f32c(q_noise, self.device)
        qa = (C.c_float * n)(*[float(v) for v in q_sqrt_ac])
        qb = (C.c_float * n)(*[float(v) for v in q_sqrt_1m_ac])
        qm = _lib.SampleMaskC(x0.data_ptr(), mask.data_ptr(), mb, mc, C.cast(qa, C.POINTER(C.c_float)), C.cast(qb, C.POINTER(C.c_float)),
                              q_noise.data_ptr())
        return qm, (x0, mask, q_noise, qa, qb)

    def q_sample_blend(self, x0: torch.Tensor, noise: torch.Tensor, sqrt_ac: float, sqrt_1m_ac: float,
                       mask: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(sqrt_ac x0 + sqrt_1m_ac noise) * mask + (1 - mask) * x on the device (mkd_q_sample_blend); mask None: the q_sample alone.
        x0, noise, x [B,C,h,w]; mask [1|B, 1|C, h, w]."""
        x0 = _f32c(x0, self.device)
        noise = _f32c(noise, self.device)
        if x0.dim() != 4 or tuple(noise.shape) != tuple(x0.shape):
            raise ValueError(f'x0 and noise must be equal [B,C,h,w] tensors, got {tuple(x0.shape)} and {tuple(noise.shape)}')
        B, Cn, h, w = x0.shape
        mb = mc = 1
        if mask is not None:
            if x is None or tuple(x.shape) != tuple(x0.shape):
                raise ValueError('a masked blend needs x of the shape of x0')
            mb, mc = self._mask_geometry(mask, B, Cn, (h, w))
            mask = _f32c(mask, self.device)
            x = _f32c(x, self.device)
        else:
            x = None
        out = torch.empty_like(x0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_q_sample_blend(C.c_void_p(x0.data_ptr()), C.c_void_p(noise.data_ptr()), float(sqrt_ac), float(sqrt_1m_ac),
                                                   C.c_void_p(_ptr(mask)), mb, mc, C.c_void_p(_ptr(x)), C.c_void_p(out.data_ptr()),
                                                   B, Cn, h * w, C.c_void_p(_stream())), 'mkd_q_sample_blend')
        return out

    def latent_mask_from_labels(self, seg: torch.Tensor, classes: Iterable[int] = (0, 11, 12), factor: int = 8,
                                threshold: float = 0.5) -> torch.Tensor:
        """Label map [B,H,W] or [B,1,H,W] (uint8, labels 0..63) -> [B,1,H/factor,W/factor] fp32: the fraction of each factor x factor
        block whose label is in ``classes`` (F.interpolate(mode='area') of the binary mask); threshold > 0: that fraction >= threshold."""
        if seg.dim() == 4 and seg.shape[1] == 1:
            seg = seg[:, 0]
        if seg.dim() != 3:
            raise ValueError(f'seg must be [B,H,W] or [B,1,H,W], got {tuple(seg.shape)}')
        if seg.dtype != torch.uint8:
            if seg.is_floating_point() or int(seg.min()) < 0 or int(seg.max()) > 255:
                raise ValueError('seg must hold integer labels 0..255')
            seg = seg.to(torch.uint8)
        bits = 0
        for c in classes:
            if not 0 <= int(c) < 64:
                raise ValueError(f'class {c} outside 0..63')
            bits |= 1 << int(c)
        B, H, W = seg.shape
        if factor < 1 or H % factor or W % factor:
            raise ValueError(f'seg {H}x{W} is not a multiple of factor {factor}')
        lab = seg.to(self.device).contiguous()
        out = torch.empty((B, 1, H // factor, W // factor), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_latent_mask_from_labels(C.c_void_p(lab.data_ptr()), B, H, W, C.c_uint64(bits), int(factor),
                                                            float(threshold), C.c_void_p(out.data_ptr()), C.c_void_p(_stream())),
                       'mkd_latent_mask_from_labels')
        return out

    def paste_background(self, image: torch.Tensor, src: torch.Tensor, seg: Optional[torch.Tensor] = None,
                         classes: Iterable[int] = (0, 11, 12), feather: int = 0, mask: Optional[torch.Tensor] = None,
                         return_alpha: bool = False):
        """Pixel-space background paste after the decode (include/mkd.h mkd_paste_background): ``image`` (the decoded sample) and ``src``
        (the source), fp32 [B,C,H,W] in [-1, 1] -> clamp((a (src + 1) / 2 + (1 - a) (image + 1) / 2) 2 - 1), the reference's
        Fixbackground.get_target.  The keep weight a comes from exactly one of ``seg`` (label map [B,fH,fW] or [B,1,fH,fW], f = 1..8
        derived from the shapes: the fraction of ``classes`` in the (2 feather + 1)^2 pixel window, feather 0..16) and ``mask`` (fp32
        [1|B,1,H,W], read as is).  Returns the pasted image, with ``return_alpha`` also a as [B,1,H,W]."""
        if (seg is None) == (mask is None):
            raise ValueError('paste_background needs exactly one of seg and mask')
        if image.dim() != 4 or tuple(src.shape) != tuple(image.shape):
            raise ValueError(f'image and src must be equal [B,C,H,W] tensors, got {tuple(image.shape)} and {tuple(src.shape)}')
        B, Cn, H, W = (int(v) for v in image.shape)
        if not 1 <= Cn <= 8 or not 1 <= B <= 65535 or H < 1 or W < 1 or H * W > 1 << 24:
            raise ValueError(f'paste_background: batch 1..65535, channels 1..8, H * W <= 2^24, got {tuple(image.shape)}')
        rho = int(feather)
        if not 0 <= rho <= 16:
            raise ValueError(f'feather must be 0..16 image pixels, got {feather}')
        lab = mk = None
        bits, factor, mb = 0, 1, 1
        if seg is not None:
            if seg.dim() == 4 and seg.shape[1] == 1:
                seg = seg[:, 0]
            if seg.dim() != 3:
                raise ValueError(f'seg must be [B,H,W] or [B,1,H,W], got {tuple(seg.shape)}')
            if seg.dtype != torch.uint8:
                if seg.is_floating_point() or int(seg.min()) < 0 or int(seg.max()) > 255:
                    raise ValueError('seg must hold integer labels 0..255')
                seg = seg.to(torch.uint8)
            for c in classes:
                if not 0 <= int(c) < 64:
                    raise ValueError(f'class {c} outside 0..63')
                bits |= 1 << int(c)
            factor = int(seg.shape[-1]) // W
            if seg.shape[0] != B or not 1 <= factor <= 8 or (int(seg.shape[-2]), int(seg.shape[-1])) != (factor * H, factor * W):
                raise ValueError(f'seg {tuple(seg.shape)} is not [B = {B}] label maps at an integer multiple 1..8 of the image {H}x{W}')
            lab = seg.to(self.device).contiguous()
        else:
            if rho:
                raise ValueError('feather applies to a label map only: a mask is read as is')
            if mask.dim() != 4 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (1, H, W):
                raise ValueError(f'mask must be [1 or {B}, 1, {H}, {W}], got {tuple(mask.shape)}')
            mk = _f32c(mask, self.device)
            mb = int(mk.shape[0])
        image = _f32c(image, self.device)
        src = _f32c(src, self.device)
        out = torch.empty_like(image)
        alpha = torch.empty((B, 1, H, W), device=self.device, dtype=torch.float32) if return_alpha else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_paste_background(C.c_void_p(image.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(_ptr(lab)),
                                                     C.c_uint64(bits), factor, rho, C.c_void_p(_ptr(mk)), mb, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(_ptr(alpha)), B, Cn, H, W, C.c_void_p(_stream())), 'mkd_paste_background')
        return (out, alpha) if return_alpha else out

    def _to_dev(self, ts, rank: int):
        """one tensor, a stacked batch or a list (photo.as_list) -> a list on this engine's device; None stays None"""
        from . import photo
        return None if ts is None else [t.to(self.device) for t in photo.as_list(ts, rank)]

    def crop_resize(self, photos, boxes, size: int, labels=None, want_u8: bool = False):
        """Full-resolution photos in (include/mkd.h mkd_crop_resize; photo.crop_resize on this engine's device): uint8 [H,W,3]
        photos and their boxes (x0, y0, w, h) -> Cropped(img01 [B,3,S,S], labels [B,S,S] or None, u8 [B,S,S,3] or None), the bytes
        of Pillow's antialiased bilinear resize of each box."""
        from . import photo
        return photo.crop_resize(self._to_dev(photos, 3), boxes, size, labels=self._to_dev(labels, 2), want_u8=want_u8)

    def paste_photos(self, photos, boxes, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None,
                     guided=None):
        """Full-resolution photos out (include/mkd.h mkd_paste_photo; photo.paste_photos): the decoded samples pasted into the
        device photos IN PLACE, inside their boxes, with the photos' fine detail kept.  ``weights`` [B,wh,ww]: one photo-wide weight
        plane per photo (mkd_paste_photo_weighted)."""
        from . import photo
        return photo.paste_photos(photos, boxes, samples, src01, feather, weights, guided)

    def crop_regions(self, photos, regions, size: int, labels=None):
        """crop_resize for a batch whose regions may be photo.Frame's (photo.crop_regions on this engine's device): a rolled frame is
        cropped along itself (include/mkd.h mkd_crop_frame), a batch without one is the crop_resize call above"""
        from . import photo
        return photo.crop_regions(self._to_dev(photos, 3), regions, size, labels=self._to_dev(labels, 2))

    def paste_regions(self, photos, regions, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None,
                      guided=None):
        """paste_photos for a batch whose regions may be photo.Frame's (photo.paste_regions; include/mkd.h mkd_paste_frame)"""
        from . import photo
        return photo.paste_regions(photos, regions, samples, src01, feather, weights, guided)

    def temporal_diff(self, t: torch.Tensor, s01: torch.Tensor, D_in: torch.Tensor, Y_in: torch.Tensor, slot_in, D_out: torch.Tensor,
                      Y_out: torch.Tensor, slot_out, filt, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Video clips (include/mkd.h mkd_temporal_diff; video.temporal_diff): the makeup difference of the faces of one frame step
        filtered over time, between the decode and the paste; one launch"""
        from . import video
        return video.temporal_diff(t, s01, D_in, Y_in, slot_in, D_out, Y_out, slot_out, filt, out)

    def motion_warp(self, s01: torch.Tensor, D_in: torch.Tensor, Y_in: torch.Tensor, slot_in, D_w: torch.Tensor, Y_w: torch.Tensor, ms,
                    vec_out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Video clips (include/mkd.h mkd_motion_warp; video.motion_warp): the previous state of the faces of one frame step fetched
        through one block-matched integer vector per block, in front of temporal_diff; one launch"""
        from . import video
        return video.motion_warp(s01, D_in, Y_in, slot_in, D_w, Y_w, ms, vec_out)

    def eps_profile(self, x: torch.Tensor, t: torch.Tensor, csv_path: Optional[str] = None) -> Dict[str, Dict[str, float]]:
        """One eps with HIP events around every launch group -> {kernel class: {ms, flops, launches, bytes, ms_b2b}}: ``bytes`` =
        algorithmic HBM bytes of the memory-bound classes, ``ms_b2b`` = the class's launches replayed back to back between one
        event pair (no per-launch event overhead)."""
        x = _f32c(x, self.device)
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((self.batch, self.cfg.out_channels, *self.latent_hw), device=self.device, dtype=torch.float32)
        n = self.lib.mkd_kind_count()
        ms = (C.c_double * n)(); fl = (C.c_double * n)(); ln = (C.c_int * n)(); by = (C.c_double * n)(); b2b = (C.c_double * n)()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_eps_profile2(self._ctx, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()),
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(_stream()), ms, fl, ln, by, b2b,
                                                 None if csv_path is None else csv_path.encode()), 'mkd_eps_profile2')
        return {self.lib.mkd_kind_name(k).decode(): {'ms': ms[k], 'flops': fl[k], 'launches': ln[k], 'bytes': by[k], 'ms_b2b': b2b[k]}
                for k in range(n)}

    # ---- introspection -----------------------------------------------------------------------------
    def eps_flops(self) -> float:
        return float(self.lib.mkd_eps_flops(self._ctx))

    def eps_launches(self) -> int:
        return int(self.lib.mkd_eps_launches(self._ctx))

    def step_launches(self, use_graph: bool = True, cfg: bool = False, rescale: bool = False, per_sample: bool = False) -> int:
        """Kernel launches of one DDIM step inside ``sample`` (time embedding hoisted out of the loop), as that loop is run;
        ``rescale``: a guided step with guidance rescale (its factor launch); ``per_sample``: a step of ``sample_rows``."""
        if per_sample:
            if rescale:
                raise ValueError('guidance rescale is not combined with per-sample rows')
            return int(self.lib.mkd_step_launches_ex(self._ctx, int(use_graph), _lib.STEP_PER_SAMPLE | int(bool(cfg))))
        return int(self.lib.mkd_step_launches_ex(self._ctx, int(use_graph), 2 if (cfg and rescale) else int(bool(cfg))))

    def device_bytes(self) -> int:
        return int(self.lib.mkd_device_bytes(self._ctx))
