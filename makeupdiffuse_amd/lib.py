"""ctypes binding of libmkd.so (include/mkd.h).  There is NO fallback: a missing library or a
missing GPU is an error, never a silent CPU path."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MKD_LIB_PATH') or os.path.join(HERE, 'libmkd.so')      # override: A/B experiments only

ABI_VERSION = 1


class MkdError(RuntimeError):
    pass


class VaeConfigC(C.Structure):
    _fields_ = [('z_channels', C.c_int32), ('embed_dim', C.c_int32), ('ch', C.c_int32), ('n_levels', C.c_int32),
                ('ch_mult', C.c_int32 * 8), ('num_res_blocks', C.c_int32), ('out_ch', C.c_int32)]


class ClipConfigC(C.Structure):
    _fields_ = [('vocab_size', C.c_int32), ('max_positions', C.c_int32), ('width', C.c_int32), ('layers', C.c_int32),
                ('heads', C.c_int32), ('intermediate', C.c_int32), ('ln_eps', C.c_float)]


class NetConfigC(C.Structure):
    _fields_ = [
        ('in_channels', C.c_int32), ('out_channels', C.c_int32), ('hint_channels', C.c_int32),
        ('model_channels', C.c_int32), ('num_res_blocks', C.c_int32), ('n_levels', C.c_int32),
        ('channel_mult', C.c_int32 * 8), ('n_attention_resolutions', C.c_int32),
        ('attention_resolutions', C.c_int32 * 8), ('num_heads', C.c_int32),
        ('transformer_depth', C.c_int32), ('context_dim', C.c_int32), ('hint_widths', C.c_int32 * 7),
    ]


class ParserConfigC(C.Structure):
    _fields_ = [('n_classes', C.c_int32), ('widths', C.c_int32 * 4), ('blocks', C.c_int32 * 4), ('cp_channels', C.c_int32),
                ('ffm_channels', C.c_int32), ('bn_eps', C.c_float), ('mean', C.c_float * 3), ('std', C.c_float * 3)]


class PhotoDescC(C.Structure):
    _fields_ = [('pixels', C.c_void_p), ('pitch_bytes', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32),
                ('bw', C.c_int32), ('bh', C.c_int32), ('labels', C.c_void_p)]


class PhotoFrameDescC(C.Structure):
    """mkd_photo_frame_desc: a photo and an oriented square in it"""
    _fields_ = [('pixels', C.c_void_p), ('pitch_bytes', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('cx', C.c_double), ('cy', C.c_double),
                ('side', C.c_double), ('c', C.c_double), ('s', C.c_double), ('labels', C.c_void_p)]


class FaceFrameC(C.Structure):
    """mkd_face_frame (48 bytes)"""
    _fields_ = [('n_a', C.c_int32), ('n_b', C.c_int32), ('cq', C.c_int32), ('sq', C.c_int32), ('umin', C.c_int64), ('umax', C.c_int64),
                ('vmin', C.c_int64), ('vmax', C.c_int64)]


class SampleMaskC(C.Structure):
    _fields_ = [('x0', C.c_void_p), ('mask', C.c_void_p), ('mask_batch', C.c_int32), ('mask_channels', C.c_int32),
                ('sqrt_alphas_cumprod', C.POINTER(C.c_float)), ('sqrt_one_minus_alphas_cumprod', C.POINTER(C.c_float)),
                ('noise', C.c_void_p)]


class SampleExtrasC(C.Structure):
    _fields_ = [('log_every_t', C.c_int32), ('rows', C.c_int32), ('trace_x', C.c_void_p), ('trace_x0', C.c_void_p),
                ('guidance_rescale', C.c_float)]


class SampleRowC(C.Structure):
    """mkd_sample_row: one sample's request of a per-sample call (host tables)"""
    _fields_ = [('n_steps', C.c_int32), ('cfg_scale', C.c_float), ('timesteps', C.POINTER(C.c_int64)),
                ('alphas', C.POINTER(C.c_float)), ('alphas_prev', C.POINTER(C.c_float)), ('sqrt_one_minus_alphas', C.POINTER(C.c_float)),
                ('sigmas', C.POINTER(C.c_float)), ('dpm', C.POINTER(C.c_float))]


class StepRowC(C.Structure):
    """mkd_step_row: one entry of the per-sample step table (64 bytes)"""
    _fields_ = [('t', C.c_int64), ('coef', C.c_float * 4), ('sigma', C.c_float), ('dpm', C.c_float * 6), ('temb_row', C.c_int32),
                ('active', C.c_int32), ('scale', C.c_float)]


MAX_STEPS = 1024          # MKD_MAX_STEPS
STEP_PER_SAMPLE = 4       # MKD_STEP_PER_SAMPLE

_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_L = C.c_int64

# name -> (restype, argtypes); every symbol include/mkd.h declares
SIGNATURES = {
    'mkd_last_error': (C.c_char_p, []),
    'mkd_abi_version': (_I, []),
    'mkd_grouped_launches_available': (_I, []),
    'mkd_ctx_create': (_I, [C.POINTER(NetConfigC), C.POINTER(_P)]),
    'mkd_ctx_destroy': (None, [_P]),
    'mkd_load_weight': (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_L)]),
    'mkd_weights_finalize': (_I, [_P]),
    'mkd_param_count': (_L, [_P, _I]),
    'mkd_param_total': (_I, [_P]),
    'mkd_param_name': (C.c_char_p, [_P, _I]),
    'mkd_param_shape': (_I, [_P, _I, C.POINTER(_L)]),
    'mkd_ctx_set_option': (_I, [_P, C.c_char_p, C.c_double]),
    'mkd_ctx_get_option': (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    'mkd_debug_tfm_trace': (_I, [_P]),
    'mkd_debug_attn_trace': (_I, [_P]),
    'mkd_live_contexts': (_I, []),
    'mkd_prepare': (_I, [_P, _I, _I, _I, _P, _P, C.POINTER(_F), _I, _P]),
    'mkd_prepare_interp': (_I, [_P, _I, _I, _I, _P, _P, _P, _P, C.POINTER(_F), _I, _P]),
    'mkd_prepare_regions': (_I, [_P, _I, _I, _I, C.POINTER(_P), _I, _P, _P, C.POINTER(_F), _I, _P]),
    'mkd_region_weights': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    'mkd_region_blend_bf16': (_I, [C.POINTER(_P), _P, _P, _I, _I, _I, _I, _P]),
    'mkd_debug_hint_embedding': (_I, [_P, _P, _P]),
    'mkd_debug_vae_attn': (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    'mkd_eps': (_I, [_P, _P, _P, _P, _P]),
    'mkd_ddim_step': (_I, [_P, _P, _P, _F, _F, _F, _F, _F, _P, _F, _P, _P, _L, _P]),
    'mkd_ddim_step_ex': (_I, [_P, _P, _P, _F, _F, _F, _F, _F, _P, _F, _P, _I, _P, _P, _L, _P]),
    'mkd_cfg_rescale_factor': (_I, [_P, _P, _F, _F, _I, _I, _P, _P]),
    'mkd_sample_log_rows': (_I, [_I, _I]),
    'mkd_sample': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _F, _P, _I, _P]),
    'mkd_sample_eta': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _P, _F, _F, _P, _I, _P]),
    'mkd_sample_masked': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _P, _F,
                               C.POINTER(SampleMaskC), _F, _P, _I, _P]),
    'mkd_sample_masked_ex': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _P, _F,
                                  C.POINTER(SampleMaskC), C.POINTER(SampleExtrasC), _F, _P, _I, _P]),
    'mkd_q_sample_blend': (_I, [_P, _P, _F, _F, _P, _I, _I, _P, _P, _I, _I, _I, _P]),
    'mkd_dpmpp_table': (_I, [_I, C.POINTER(_F), C.POINTER(_F), _I, _I, C.POINTER(_F), C.POINTER(_I)]),
    'mkd_dpmpp_step': (_I, [_P, _P, _P, _F, C.POINTER(_F), _P, _P, _P, _P, _L, _P]),
    'mkd_dpmpp_step_ex': (_I, [_P, _P, _P, _F, C.POINTER(_F), _P, _P, _P, _I, _P, _P, _L, _P]),
    'mkd_sample_dpmpp_ex': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), _I, _I, C.POINTER(SampleMaskC),
                                 C.POINTER(SampleExtrasC), _F, _P, _I, _P]),
    'mkd_sample_dpmpp': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), _I, _I, C.POINTER(SampleMaskC), _F, _P, _I, _P]),
    'mkd_unipc_table': (_I, [_I, C.POINTER(_F), C.POINTER(_F), _I, _I, _I, C.POINTER(_F), C.POINTER(_I)]),
    'mkd_unipc_step': (_I, [_P, _P, _P, _P, _F, C.POINTER(_F), _P, _P, _P, _P, _P, _P, _L, _P]),
    'mkd_unipc_step_ex': (_I, [_P, _P, _P, _P, _F, C.POINTER(_F), _P, _P, _P, _P, _I, _P, _P, _P, _L, _P]),
    'mkd_sample_unipc_ex': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), _I, _I, _I, C.POINTER(SampleMaskC),
                                 C.POINTER(SampleExtrasC), _F, _P, _I, _P]),
    'mkd_sample_unipc': (_I, [_P, _P, _I, _I, C.POINTER(_L), C.POINTER(_F), C.POINTER(_F), _I, _I, _I, C.POINTER(SampleMaskC), _F, _P, _I, _P]),
    'mkd_step_table': (_I, [C.POINTER(SampleRowC), _I, _I, C.POINTER(StepRowC), C.POINTER(_I), C.POINTER(_L), C.POINTER(_I)]),
    'mkd_sample_rows': (_I, [_P, _P, _I, C.POINTER(SampleRowC), _I, _P, _F, C.POINTER(SampleMaskC), C.POINTER(SampleExtrasC), _P, _I, _P]),
    'mkd_ddim_step_rows': (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _P]),
    'mkd_dpmpp_step_rows': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    'mkd_latent_mask_from_labels': (_I, [_P, _I, _I, _I, C.c_uint64, _I, _F, _P, _P]),
    'mkd_paste_background': (_I, [_P, _P, _P, C.c_uint64, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    'mkd_region_mask_from_labels': (_I, [_P, _I, _I, _I, C.c_uint64, C.c_uint64, _I, _P, _P, _P, _P]),
    'mkd_label_components_scratch_bytes': (C.c_size_t, [_I, _I, _I]),
    'mkd_label_components': (_I, [_P, _I, _I, _I, C.c_uint64, _I, _I, _P, _P, _P, _P, _P]),
    'mkd_owner_map_scratch_bytes': (C.c_size_t, [_I, _I, _I]),
    'mkd_owner_map': (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    'mkd_owner_weights': (_I, [_P, _I, _I, _I, C.POINTER(C.c_int32), _I, _I, _P, _P]),
    'mkd_hist_match_scratch_bytes': (C.c_size_t, [_I]),
    'mkd_hist_match_launches': (_I, [_I, _I]),
    'mkd_hist_match': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    'mkd_pgt_compose': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    'mkd_pgt_launches': (_I, []),
    'mkd_pgt_warp': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    'mkd_pgt_warp_launches': (_I, []),
    'mkd_region_points': (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    'mkd_region_points_scratch_bytes': (C.c_size_t, [_I]),
    'mkd_region_points_launches': (_I, []),
    'mkd_tps_solve': (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    'mkd_tps_solve_launches': (_I, []),
    'mkd_crop_resize_scratch_bytes': (C.c_size_t, [C.POINTER(PhotoDescC), _I, _I]),
    'mkd_crop_resize': (_I, [C.POINTER(PhotoDescC), _I, _I, _P, _P, _P, _P, _P]),
    'mkd_resize_coeffs': (_I, [_I, _I, _I, _I, _P, _P, _P]),
    'mkd_paste_photo': (_I, [C.POINTER(PhotoDescC), _I, _I, _P, _P, _I, _P]),
    'mkd_paste_photo_weighted': (_I, [C.POINTER(PhotoDescC), _I, _I, _P, _P, _I, _P, _I, _I, _P]),
    'mkd_paste_photo_guided': (_I, [C.POINTER(PhotoDescC), _I, _I, _P, _P, _I, _P, _I, _I, _I, _F, _P]),
    'mkd_crop_frame': (_I, [C.POINTER(PhotoFrameDescC), _I, _I, _P, _P, _P, _P]),
    'mkd_paste_frame': (_I, [C.POINTER(PhotoFrameDescC), _I, _I, _P, _P, _I, _P, _I, _I, _P]),
    'mkd_paste_frame_guided': (_I, [C.POINTER(PhotoFrameDescC), _I, _I, _P, _P, _I, _P, _I, _I, _I, _F, _P]),
    'mkd_temporal_diff': (_I, [_P, _P, _I, _I, _P, _P, C.POINTER(C.c_int32), _P, _P, C.POINTER(C.c_int32), _I, _F, _F, _I, _P, _P]),
    'mkd_motion_warp': (_I, [_P, _I, _I, _P, _P, C.POINTER(C.c_int32), _I, _I, _I, _I, _P, _P, _P, _P]),
    'mkd_face_frames_scratch_bytes': (C.c_size_t, [_I, _I]),
    'mkd_face_frames': (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(C.c_int32), C.c_uint64, C.c_uint64, _I, _P, _P, _P]),
    'mkd_vae_configure': (_I, [_P, C.POINTER(VaeConfigC)]),
    'mkd_vae_finalize': (_I, [_P]),
    'mkd_decode': (_I, [_P, _P, _I, _I, _I, _F, _P, _P]),
    'mkd_decode_flops': (C.c_double, [_P]),
    'mkd_vae_encoder_configure': (_I, [_P, C.POINTER(VaeConfigC)]),
    'mkd_vae_encoder_finalize': (_I, [_P]),
    'mkd_encode': (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P, _P]),
    'mkd_encode_flops': (C.c_double, [_P]),
    'mkd_clip_configure': (_I, [_P, C.POINTER(ClipConfigC)]),
    'mkd_clip_finalize': (_I, [_P]),
    'mkd_clip_encode': (_I, [_P, _P, _I, _I, _P, _P]),
    'mkd_kind_count': (_I, []),
    'mkd_kind_name': (C.c_char_p, [_I]),
    'mkd_eps_profile': (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_I), C.c_char_p]),
    'mkd_eps_profile2': (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_I), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), C.c_char_p]),
    'mkd_eps_flops': (C.c_double, [_P]),
    'mkd_eps_launches': (_I, [_P]),
    'mkd_step_launches': (_I, [_P]),
    'mkd_step_launches_ex': (_I, [_P, _I, _I]),
    'mkd_device_bytes': (_L, [_P]),
    'mkd_gemm_bf16': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _I, _F, _I, _P, _I, _I, _I, _I, _I,
                           _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mkd_conv3x3_fold_bf16': (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mkd_conv3x3_down_bf16': (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'mkd_gemm_gnstat_bf16': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _I, _F, _I, _P, _I, _I, _I, _I, _I,
                                  _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    'mkd_gemm_groupnorm_bf16': (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _P, _I, _F, _P, _I, _I, _I, _I, _I,
                                     _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _F, _I, _P, _I, _P]),
    'mkd_gn_colstats': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    'mkd_gn_apply_stats': (_I, [_P, _I, _P, _P, _F, _I, _P, _I, _I, _I, _I, _P, _P]),
    'mkd_gemm_force_tile': (_I, [_I]),
    'mkd_gemm_tile_info': (_I, [_I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_char_p)]),
    'mkd_gemm_set_xcd_mode': (_I, [_I]),
    'mkd_debug_poison': (_I, [_P]),
    'mkd_gemm_set_override': (_I, [_I, _I, _I, _I, _I, _I, _I, _I]),
    'mkd_gemm_cfg_supported': (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I]),
    'mkd_fold_layernorm': (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _P, _P, _P]),
    'mkd_gemm_ln_bf16': (_I, [_P, _I, _P, _I, _P, _P, _P, _I, _F, _I, _P, _I, _I, _I, _I, _P]),
    'mkd_gemm_rowstats_bf16': (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P, _I, C.POINTER(_I), _P]),
    'mkd_groupnorm': (_I, [_P, _I, _P, _P, _F, _I, _P, _I, _I, _I, _I, _I, _P]),
    'mkd_tfm_tail_create': (_I, [_I] + [_P] * 15 + [C.POINTER(_P)]),
    'mkd_tfm_tail_destroy': (None, [_P]),
    'mkd_tfm_tail_set_context': (_I, [_P, _P, _I, _I, _I, _P]),
    'mkd_tfm_tail_run': (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    'mkd_tfm_head_create': (_I, [_I] + [_P] * 9 + [C.POINTER(_P)]),
    'mkd_tfm_head_destroy': (None, [_P]),
    'mkd_tfm_head_run': (_I, [_P, _P, _I, _F, _P, _P, _I, _I, _P]),
    'mkd_layernorm': (_I, [_P, _P, _P, _F, _P, _I, _I, _P]),
    'mkd_layernorm_ld': (_I, [_P, _I, _P, _P, _F, _P, _I, _I, _P]),
    'mkd_attention': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _F, _P]),
    'mkd_attention_causal': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _F, _P]),
    'mkd_geglu': (_I, [_P, _P, _I, _I, _P]),
    'mkd_softmax_rows': (_I, [_P, _P, _I, _I, _P]),
    'mkd_vae_enc_tail': (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _I, _I, _I, _P]),
    'mkd_post_quant': (_I, [_P, _P, _P, _F, _P, _I, _I, _I, _P]),
    'mkd_timestep_embedding': (_I, [_P, _P, _I, _I, _P]),
    'mkd_clip_embed': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'mkd_blend_bf16': (_I, [_P, _P, _P, _P, _L, _I, _P]),
    'mkd_conv3x3_direct': (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mkd_pack_conv_weight': (_I, [_P, _P, _I, _I, _I, _I, _P]),
    'mkd_parser_create': (_I, [C.POINTER(ParserConfigC), C.POINTER(_P)]),
    'mkd_parser_destroy': (None, [_P]),
    'mkd_parser_param_total': (_I, [_P]),
    'mkd_parser_param_name': (C.c_char_p, [_P, _I]),
    'mkd_parser_param_shape': (_I, [_P, _I, C.POINTER(_L)]),
    'mkd_parser_param_count': (_L, [_P]),
    'mkd_parser_load_weight': (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_L)]),
    'mkd_parser_finalize': (_I, [_P]),
    'mkd_parser_logits': (_I, [_P, _P, _I, _I, _I, _P, _P]),
    'mkd_parser_parse': (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    'mkd_parser_flops': (C.c_double, [_P, _I, _I]),
    'mkd_parser_launches': (_I, [_P]),
    'mkd_parse_labels': (_I, [_P, _L, _L, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    'mkd_parser_stem': (_I, [_P, _P, _P, C.POINTER(_F), C.POINTER(_F), _P, _P, _I, _I, _I, _I, _P]),
    'mkd_channel_gate': (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P]),
    'mkd_gate_apply_bf16': (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'mkd_noise_fill': (_I, [_P, _P, _I, C.c_uint32, C.c_uint32, _I, _L, _I, _P, _P]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen libmkd.so and bind every declared symbol; raises MkdError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MkdError(f'{LIB_PATH} is missing: build it with `python -m makeupdiffuse_amd.build` '
                       '(there is no CPU fallback for the hot path)')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.mkd_abi_version() != ABI_VERSION:
        raise MkdError(f'libmkd.so ABI {lib.mkd_abi_version()} != binding ABI {ABI_VERSION}: rebuild')
    _lib = lib
    return lib


def check(rc: int, what: str = '') -> None:
    if rc != 0:
        msg = load().mkd_last_error()
        raise MkdError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')


def tile_table() -> list:
    """[(tile_m, tile_n, lds_staged_conv, name)] of every GEMM tile configuration, in index order (mkd_gemm_tile_info; needs no GPU)."""
    lib = load()
    m, n, patch, name = _I(), _I(), _I(), C.c_char_p()
    rows = []
    for cfg in range(lib.mkd_gemm_tile_info(-1, None, None, None, None)):
        lib.mkd_gemm_tile_info(cfg, C.byref(m), C.byref(n), C.byref(patch), C.byref(name))
        rows.append((m.value, n.value, bool(patch.value), name.value.decode()))
    return rows
