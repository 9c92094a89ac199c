"""ctypes binding of libspa3d_hip.so (include/spa3d.h).  Fails loudly when the library is missing:
there is no CPU fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libspa3d_hip.so')

F32, BF16, F16 = 0, 1, 2  # spa3d_config::precision / op dtype (include/spa3d.h)


class Config(C.Structure):
  _fields_ = [
      ('num_output_frames', C.c_int32), ('num_latent_tokens', C.c_int32), ('latent_token_dim', C.c_int32),
      ('num_frequencies', C.c_int32), ('track_scale_factor', C.c_float), ('time_scale_factor', C.c_float),
      ('track_token_dim', C.c_int32), ('encoder_latent_dim', C.c_int32), ('decoder_num_channels', C.c_int32),
      ('dino_feature_dim', C.c_int32), ('depth_feature_dim', C.c_int32), ('num_heads', C.c_int32),
      ('qkv_size', C.c_int32), ('enc_mlp', C.c_int32), ('enc_layers', C.c_int32), ('t2l_mlp', C.c_int32),
      ('t2l_layers', C.c_int32), ('dec_mlp', C.c_int32), ('dec_layers', C.c_int32), ('ro_mlp', C.c_int32),
      ('ro_layers', C.c_int32), ('precision', C.c_int32), ('model_kind', C.c_int32),
  ]


class Batch(C.Structure):
  _fields_ = [
      ('B', C.c_int32), ('N', C.c_int32), ('Q', C.c_int32), ('T', C.c_int32),
      ('support_tracks', C.c_void_p), ('support_tracks_visible', C.c_void_p), ('query_points', C.c_void_p),
      ('boundary_frame', C.c_void_p), ('dino_features', C.c_void_p), ('depth_features', C.c_void_p),
      ('noise', C.c_void_p), ('discretize', C.c_int32), ('query_tracks', C.c_void_p),
      ('query_tracks_visible', C.c_void_p),
  ]


class Outputs(C.Structure):
  _fields_ = [('tracks', C.c_void_p), ('visible_logits', C.c_void_p), ('certain_logits', C.c_void_p),
              ('latents', C.c_void_p)]


class Scores(C.Structure):
  """spa3d_scores (include/spa3d.h): thresholds by value, device pointers for the optional sample scale and the three result tensors."""
  _fields_ = [('num_thresholds', C.c_int32), ('thresholds', C.c_float * 8), ('sample_scale', C.c_void_p), ('query_stats', C.c_void_p),
              ('sample_stats', C.c_void_p), ('frame_err', C.c_void_p)]


class LossConfig(C.Structure):
  """spa3d_loss_config (include/spa3d.h): eight 4-byte fields, 32 bytes."""
  _fields_ = [('l1_weight', C.c_float), ('bce_weight', C.c_float), ('position_kind', C.c_int32), ('huber_delta', C.c_float),
              ('axis_weight', C.c_float * 3), ('bce_pos_weight', C.c_float)]


class ParamGroup(C.Structure):
  """spa3d_param_group (include/spa3d.h): one range [begin, end) of the optimizer's buffers with its two multipliers, 24 bytes."""
  _fields_ = [('begin', C.c_int64), ('end', C.c_int64), ('lr_scale', C.c_float), ('wd_scale', C.c_float)]


class TapVid3D(C.Structure):
  """spa3d_tapvid3d (include/spa3d.h): the scaling mode, the threshold table switch, then device pointers."""
  _fields_ = [('scaling', C.c_int32), ('fixed_thresholds', C.c_int32), ('intrinsics', C.c_void_p), ('query_stats', C.c_void_p),
              ('sample_stats', C.c_void_p), ('scale', C.c_void_p), ('row_scale', C.c_void_p), ('ratio', C.c_void_p)]


class Render(C.Structure):
  """spa3d_render (include/spa3d.h): one clip's sizes, device pointers and drawing options."""
  _fields_ = [('N', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('video', C.c_void_p), ('out', C.c_void_p), ('tracks', C.c_void_p),
              ('coords', C.c_int32), ('intrinsics', C.c_void_p), ('extrinsics', C.c_void_p), ('resize_h', C.c_int32), ('resize_w', C.c_int32),
              ('scores', C.c_void_p), ('visible', C.c_void_p), ('normalize', C.c_int32), ('use_visibility', C.c_int32), ('colour_bgr', C.c_int32),
              ('trail', C.c_int32), ('point_size', C.c_int32), ('pixels', C.c_void_p)]


class Heatmap(C.Structure):
  """spa3d_heatmap (include/spa3d.h): one clip's sizes, device pointers and the options of the map and of its overlay."""
  _fields_ = [('N', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('tracks', C.c_void_p), ('coords', C.c_int32),
              ('intrinsics', C.c_void_p), ('extrinsics', C.c_void_p), ('resize_h', C.c_int32), ('resize_w', C.c_int32), ('values', C.c_void_p),
              ('visible', C.c_void_p), ('use_visibility', C.c_int32), ('radius', C.c_int32), ('power', C.c_int32), ('map', C.c_void_p), ('weight', C.c_void_p),
              ('video', C.c_void_p), ('out', C.c_void_p), ('normalize', C.c_int32), ('lo', C.c_float), ('hi', C.c_float), ('alpha', C.c_int32),
              ('colour_bgr', C.c_int32)]


class Clip(C.Structure):
  """spa3d_clip (include/spa3d.h): one clip of spa3d_build_batch -- device pointers, except `intrinsics` (host double[4] or NULL)."""
  _fields_ = [('n_tracks', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('tracks_2d', C.c_void_p), ('tracks_3d', C.c_void_p),
              ('visible', C.c_void_p), ('depth_map', C.c_void_p), ('dino_map', C.c_void_p), ('Hp', C.c_int32), ('Wp', C.c_int32), ('dino_pool', C.c_void_p),
              ('depth_pool', C.c_void_p), ('intrinsics', C.POINTER(C.c_double)), ('n_support', C.c_int32), ('n_query', C.c_int32),
              ('support_index', C.c_void_p), ('query_index', C.c_void_p), ('query_frame', C.c_void_p)]


class Stitch(C.Structure):
  """spa3d_stitch (include/spa3d.h): sizes and the blend, the HOST plan (t0, len), then device pointers."""
  _fields_ = [('W', C.c_int32), ('N', C.c_int32), ('Tw', C.c_int32), ('TL', C.c_int32), ('NC', C.c_int32), ('blend', C.c_int32),
              ('t0', C.POINTER(C.c_int32)), ('len', C.POINTER(C.c_int32)), ('row_track', C.c_void_p), ('tracks', C.c_void_p), ('visible_logits', C.c_void_p),
              ('frame_err', C.c_void_p), ('out_tracks', C.c_void_p), ('out_visible_logits', C.c_void_p), ('out_frame_err', C.c_void_p), ('out_spread', C.c_void_p)]


class GemmArgs(C.Structure):
  """spa3d_gemm_args (include/spa3d.h): one GEMM as the planner's descriptor states it; device pointers, element strides."""
  _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('C', C.c_void_p), ('M', C.c_int64), ('N', C.c_int32), ('K', C.c_int32),
              ('sAm', C.c_int64), ('sAk', C.c_int64), ('sBk', C.c_int64), ('sBn', C.c_int64), ('sCm', C.c_int64), ('nb1', C.c_int32), ('nb2', C.c_int32),
              ('bA1', C.c_int64), ('bA2', C.c_int64), ('bB1', C.c_int64), ('bB2', C.c_int64), ('bC1', C.c_int64), ('bC2', C.c_int64),
              ('alpha', C.c_float), ('bias', C.c_void_p), ('epi', C.c_int32), ('aux', C.c_void_p), ('aux_is_residual', C.c_int32),
              ('out_f32', C.c_int32), ('accumulate', C.c_int32), ('pre_out', C.c_void_p),
              ('crow_group', C.c_int32), ('crow_skip', C.c_int32), ('brow_group', C.c_int32), ('brow_skip', C.c_int32),
              ('seg_n', C.c_int32), ('C_seg', C.c_void_p * 2), ('colsum_out', C.c_void_p),
              ('A2', C.c_void_p), ('sA2m', C.c_int64), ('K1', C.c_int32), ('arow_idx', C.c_void_p), ('crow_idx', C.c_void_p),
              ('r1_x', C.c_void_p), ('r1_w', C.c_void_p), ('Bt', C.c_void_p), ('ldBt', C.c_int64)]


EPI_NONE, EPI_GELU, EPI_MUL_GELU_GRAD = 0, 1, 2  # SPA3D_EPI_*
# SPA3D_GEMM_*: the kernel spa3d_op_gemm reports, by the planner's names (csrc/gemm_plan.hpp GemmKernel)
GEMM_KERNELS = ('Refuse', 'Generic', 'Rs', 'Ntb', 'MlpFused', 'NtEmbed', 'Nt8pp256', 'Nt8pp384', 'Nt8p256', 'Nt8p384', 'NtOcc', 'Nt',
                'Tnb', 'Tn8p256', 'Tn8p128x384', 'Tn8p384x128', 'Tn')

BLEND_MEAN, BLEND_HAT, BLEND_FIRST = 0, 1, 2  # SPA3D_BLEND_* (include/spa3d.h)
POOL_TOKEN, POOL_CLIP = 0, 1                  # SPA3D_POOL_*
PDIST_DOT, PDIST_SQDIST = 0, 1                # SPA3D_PDIST_*

_SIGS = {
    'spa3d_version': (C.c_char_p, []),
    'spa3d_create': (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    'spa3d_destroy': (C.c_int, [C.c_void_p]),
    'spa3d_last_error': (C.c_char_p, [C.c_void_p]),
    'spa3d_param_elems': (C.c_int64, [C.c_void_p]),
    'spa3d_num_leaves': (C.c_int32, [C.c_void_p]),
    'spa3d_leaf_info': (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    'spa3d_workspace_bytes': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'spa3d_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_void_p, C.POINTER(Outputs), C.c_void_p,
                               C.c_int64, C.c_void_p]),
    'spa3d_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.POINTER(Outputs), C.c_void_p, C.c_int64,
                                C.c_void_p]),
    'spa3d_loss': (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Outputs), C.c_float, C.c_void_p, C.c_void_p]),
    'spa3d_op_head_loss': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(Outputs), C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_score': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.POINTER(Scores), C.POINTER(Outputs), C.c_void_p, C.c_int64,
                              C.c_void_p]),
    'spa3d_score_folds_workspace_bytes': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    'spa3d_score_folds': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Scores), C.POINTER(Outputs),
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_score_from_preds': (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Outputs), C.POINTER(Scores), C.c_void_p]),
    'spa3d_tapvid3d_workspace_bytes': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    'spa3d_tapvid3d_from_preds': (C.c_int, [C.c_void_p, C.POINTER(Batch), C.POINTER(Outputs), C.POINTER(TapVid3D), C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_render_workspace_bytes': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32]),
    'spa3d_render_tracks': (C.c_int, [C.c_void_p, C.POINTER(Render), C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_heatmap_workspace_bytes': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32]),
    'spa3d_render_heatmap': (C.c_int, [C.c_void_p, C.POINTER(Heatmap), C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_build_batch': (C.c_int, [C.c_void_p, C.POINTER(Clip), C.POINTER(Batch), C.c_void_p]),
    'spa3d_build_windows': (C.c_int, [C.c_void_p, C.POINTER(Clip), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Batch), C.c_void_p]),
    'spa3d_stitch_windows': (C.c_int, [C.c_void_p, C.POINTER(Stitch), C.c_void_p]),
    'spa3d_motion_codes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_motion_moments_add': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'spa3d_motion_pdist': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'spa3d_motion_knn_workspace_bytes': (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    'spa3d_motion_knn': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_void_p]),
    'spa3d_motion_ball_hits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_motion_kernel_sums': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_op_median_rows': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_loss_and_grads': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_float, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.POINTER(Outputs), C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_adamw_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int64,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'spa3d_adamw_groups_workspace_bytes': (C.c_int64, [C.c_int32]),
    'spa3d_adamw_step_groups': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int64,
                                          C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(ParamGroup), C.c_int32,
                                          C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_set_option': (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    'spa3d_set_loss_scale_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'spa3d_set_counts': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'spa3d_set_loss': (C.c_int, [C.c_void_p, C.POINTER(LossConfig)]),
    'spa3d_get_loss': (C.c_int, [C.c_void_p, C.POINTER(LossConfig)]),
    'spa3d_set_point_weights': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_grad_segments': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'spa3d_trainable_range': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'spa3d_set_grad_events': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_grad_events_recorded': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'spa3d_detach': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_plan_stats': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'spa3d_prof_enable': (C.c_int, [C.c_void_p, C.c_int32]),
    'spa3d_prof_read': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    'spa3d_prof_dump': (C.c_int, [C.c_void_p, C.c_char_p]),
    'spa3d_uniform_noise': (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p]),
    'spa3d_op_sin_embed': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_linear': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_linear_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_gemm': (C.c_int, [C.POINTER(GemmArgs), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_mlp_fused': (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_layernorm': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    'spa3d_op_layernorm_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_qkv_attention': (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 3
                               + [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 3 + [C.c_int64] + [C.c_int32] * 4
                           + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_holdout': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 2 + [C.c_int64] + [C.c_int32] * 4
                                   + [C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_bwd': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 3 + [C.c_int64]
                               + [C.c_int32] * 4 + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                                       C.c_void_p]),
    'spa3d_op_attention_ragged': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 3 + [C.POINTER(C.c_int32), C.c_int64] + [C.c_int32] * 3
                                  + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_ragged_bwd': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 3 + [C.POINTER(C.c_int32), C.c_int64] + [C.c_int32] * 3
                                      + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_varlen': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 2 + [C.POINTER(C.c_int32), C.c_int64] + [C.c_int32] * 3
                                  + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_varlen_bwd': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 2 + [C.POINTER(C.c_int32), C.c_int64] + [C.c_int32] * 3
                                      + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_attention_q1': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                              + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_attention_q1_bwd': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64]
                                  + [C.c_int32] * 3 + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]),
    'spa3d_op_rank_linear': (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_rank_linear_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_colsum': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_rows': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_prune_plan': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    'spa3d_op_share_plan': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(C.c_int64), C.c_void_p]),
    'spa3d_op_share_rows': (C.c_int, [C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_int64] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_assemble_readout': (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_assemble_readout_bwd': (C.c_int, [C.c_void_p] * 2 + [C.c_int64] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_broadcast_rows': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    'spa3d_op_bcast_grad': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_vis_mean_pool': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_vis_mean_pool_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_sin_embed_scaled': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_embed_tokens': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_query_embed': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'spa3d_op_embed_maps': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_set_readout_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'spa3d_op_keymask': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'spa3d_op_sum3': (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    'spa3d_op_pack': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    'spa3d_op_transpose': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_discretize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'spa3d_op_sample_dino': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_int32, C.c_void_p]),
    'spa3d_op_sample_depth_features': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    'spa3d_op_lift_2d_to_3d': (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
}

_lib = None


def exported_symbols():
  return sorted(_SIGS)


def load():
  """dlopen the library and bind every symbol include/spa3d.h declares."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise ImportError(
        f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
        '(hipcc --offload-arch=gfx950).  The 3DSPA hot path has no CPU fallback.')
  lib = C.CDLL(LIB_PATH)
  for name, (res, args) in _SIGS.items():
    fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
    fn.restype = res
    fn.argtypes = args
  _lib = lib
  return lib


class Spa3dError(RuntimeError):
  pass


def check(rc, handle=None, what=''):
  if rc != 0:
    msg = ''
    if handle is not None:
      msg = load().spa3d_last_error(handle).decode()
    raise Spa3dError(f'{what} failed with status {rc}: {msg}')
