"""ctypes binding of libdecafnet_hip.so (the C ABI declared in include/decafnet_hip.h and the extension headers beside it).

The product path has no CPU fallback: if the shared object is missing or cannot be loaded,
``lib()`` raises and every operator fails loudly.
"""
import ctypes
import os
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCF_LIB_PATH: developer switch for A/B runs of two builds inside one GPU call (tools/); the product path is the in-tree build
SO_PATH = os.environ.get('DCF_LIB_PATH') or os.path.join(_HERE, 'libdecafnet_hip.so')
_LIB = None

c_f32p = ctypes.c_void_p      # device pointers are passed as raw addresses
c_u8p = ctypes.c_void_p
c_i32p = ctypes.c_void_p
c_i64p = ctypes.c_void_p
i32, i64, f32, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
vp = ctypes.c_void_p


class DcfConfig(ctypes.Structure):
    _fields_ = [(n, i32) for n in ('D', 'E', 'TE', 'vid_heads', 'fusion_heads', 'fusion_layers', 'n_embd_convs',
                                   'n_stem', 'n_levels', 'win', 'head_layers', 'sn')] + \
               [('sratio', f32)] + [(n, i32) for n in ('msf', 'norm', 'use_abs_pe', 'max_batch', 'gemm_mode', 'model_kind', 'second_fusion',
                                                      'text_in', 'text_layers', 'text_heads', 'text_abs_pe', 'text_bkgd',
                                                      'scat', 'sfonly', 'text_kind', 'xattn_affine', 'vid_stride', 'pool_only', 'attn_mode')]


class DcfOptimGroup(ctypes.Structure):
    """dcf_optim_group: one parameter group's hyper-parameters of dcf_optim_adam_step (a host array, passed by value with the launch)"""
    _fields_ = [(n, f32) for n in ('lr', 'weight_decay', 'b1', 'b2', 'one_minus_b1', 'one_minus_b2', 'eps', 'bc1', 'sqrt_bc2')] + [('mode', i32)]


OPTIM_CHUNK = 4096            # DCF_OPTIM_CHUNK: elements per workgroup of the dcf_optim_* kernels
OPTIM_MAX_GROUPS = 8          # DCF_OPTIM_MAX_GROUPS
OPTIM_NO_GRAD = 1             # DCF_OPTIM_NO_GRAD
OPTIM_MODES = {'adamw': 0, 'adam': 1}


# Every table below maps name -> (restype, argtypes) and belongs to one header of include/; EXTENSIONS, after the last of them, is
# the registry that says which.  The base table: ABI 12 (include/decafnet_hip.h).
SIGNATURES = {
    'dcf_last_error': (ctypes.c_char_p, []),
    'dcf_abi_version': (i32, []),
    'dcf_model_create': (i32, [ctypes.POINTER(DcfConfig), ctypes.POINTER(vp)]),
    'dcf_model_destroy': (None, [vp]),
    'dcf_model_bind': (i32, [vp, ctypes.c_char_p, c_f32p, ctypes.POINTER(i64), i32]),
    'dcf_model_set_pe': (i32, [vp, c_f32p, i64]),
    'dcf_model_set_text_pe': (i32, [vp, c_f32p, i64]),
    'dcf_text_encode': (i32, [vp, c_f32p, c_u8p, i32, c_f32p, c_u8p, vp]),
    'dcf_model_finalize': (i32, [vp, vp]),
    'dcf_numerics_status': (i32, [vp, i32, vp]),
    'dcf_numerics_status_async': (i32, [vp, vp, vp]),
    'dcf_points_per_query': (i64, [vp, i64]),
    'dcf_forward_eval': (i32, [vp, c_f32p, c_f32p, c_u8p, i64, i32, ctypes.POINTER(vp), ctypes.POINTER(vp),
                               ctypes.POINTER(i32), c_f32p, c_f32p, c_f32p, c_u8p, vp]),
    'dcf_forward_eval_videos': (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), i64, ctypes.POINTER(i32),
                                      ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(vp),
                                      c_f32p, c_f32p, c_u8p, vp]),
    'dcf_forward_train_videos': (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), i64, ctypes.POINTER(i32),
                                       ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(vp),
                                       c_f32p, c_f32p, c_f32p, c_u8p, vp]),
    'dcf_model_set_dropout': (i32, [vp, f32, f32, f32, f32, f32, i64]),
    'dcf_debug_dropout_keep': (i32, [i64, i32, i64, i64, f32, c_u8p, vp]),
    'dcf_sigmoid_focal_loss': (i32, [c_f32p, c_f32p, c_u8p, i64, f32, f32, i32, c_f32p, c_f32p, c_i32p, vp]),
    'dcf_ctr_iou_loss': (i32, [c_f32p, c_f32p, c_u8p, i64, i32, f32, c_f32p, c_f32p, c_i32p, vp]),
    'dcf_annotate_points': (i32, [c_f32p, i32, i64, i32, f64, f64, i32, i64, i32, f64, c_u8p, c_f32p, c_u8p, c_u8p, vp]),
    'dcf_point_objective': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i64, i32, f64, f64, i32, i64, i32, f64, f32, f64, i32, f32,
                                  c_f32p, f32, f32, c_f32p, c_f32p, vp]),
    'dcf_sigmoid_focal_loss_grad': (i32, [c_f32p, c_f32p, c_u8p, i64, f32, f32, i32, c_f32p, c_f32p, c_i32p, c_f32p, vp]),
    'dcf_ctr_iou_loss_grad': (i32, [c_f32p, c_f32p, c_u8p, i64, i32, f32, c_f32p, c_f32p, c_i32p, c_f32p, vp]),
    'dcf_point_objective_grad': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i64, i32, f64, f64, i32, i64, i32, f64, f32, f64, i32, f32,
                                       c_f32p, f32, f32, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, c_f32p, c_f32p, vp]),
    'dcf_forward_eval_gated': (i32, [vp, c_f32p, c_f32p, c_u8p, i64, i32, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                     ctypes.POINTER(i32), c_f32p, c_f32p, c_f32p, c_u8p, vp]),
    'dcf_hybrid_phase1': (i32, [vp, i32, c_f32p, c_f32p, c_u8p, i64, i64, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32),
                                c_f32p, c_f32p, vp]),
    'dcf_hybrid_phase2': (i32, [vp, c_f32p, c_u8p, i64, c_f32p, vp]),
    'dcf_hybrid_phase3': (i32, [vp, c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_u8p, vp]),
    'dcf_debug_copy': (i32, [vp, i32, c_f32p, i64, vp]),
    'dcf_graph_active': (i32, [vp]),
    'dcf_debug_set_option': (i32, [ctypes.c_char_p, i32]),
    'dcf_calib_mfma_rate': (i32, [i32, i32, ctypes.POINTER(i32), ctypes.POINTER(f32)]),
    'dcf_model_set_graph_mode': (i32, [vp, i32]),
    'dcf_model_set_ln_carry': (i32, [vp, i32]),
    'dcf_profile_enable': (i32, [i32]),
    'dcf_profile_report': (i64, [ctypes.c_char_p, i64]),
    'dcf_collect_segments': (i32, [c_f32p, c_f32p, c_u8p, i32, i64, i32, f32, i32, f32, c_f32p, c_f32p, c_i32p, vp]),
    'dcf_collect_segments_ext': (i32, [c_f32p, c_f32p, c_u8p, c_f32p, i32, i64, i32, f32, i32, f32, c_f32p, c_f32p, c_i32p, vp]),
    'dcf_nms_1d': (i32, [c_f32p, c_f32p, c_i32p, i32, i32, i32, f32, c_i64p, c_i32p, vp]),
    'dcf_softnms_1d': (i32, [c_f32p, c_f32p, c_i32p, i32, i32, i32, f32, f32, f32, i32, i32, c_f32p, c_i64p, c_i32p, vp]),
    'dcf_segment_voting': (i32, [c_f32p, i32, c_i32p, i32, i32, c_f32p, c_f32p, c_i32p, i32, i32, f32, i32, c_f32p, vp]),
    'dcf_op_linear': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_linear_split': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_linear_cm': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_linear_ln': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_linear_ln_carry': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, vp]),
    'dcf_op_ffn': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_linear_cm_split': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_head': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, f32, i32, vp]),
    'dcf_op_conv3': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_conv3_split': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_layernorm': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_conv_bwd_data': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_conv_bwd_weight': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, vp]),
    'dcf_op_layernorm_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_conv5s2_split': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_conv5s2_bwd_data': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_conv5s2_bwd_weight': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_xattn': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_local_attn': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_local_attn_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_dwconv3': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_dwconv3_bwd': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, vp]),
    'dcf_op_masked_maxpool': (i32, [c_f32p, c_u8p, c_f32p, c_u8p, i32, i32, i32, vp]),
    'dcf_op_masked_maxpool_bwd': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_gelu': (i32, [c_f32p, c_f32p, i64, vp]),
    'dcf_op_gelu_bwd': (i32, [c_f32p, c_f32p, c_f32p, i64, vp]),
    'dcf_op_layerscale_residual': (i32, [c_f32p, c_u8p, c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, vp]),
    'dcf_op_layerscale_residual_bwd': (i32, [c_f32p, c_f32p, c_u8p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_xattn_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_adaln': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_adaln_bwd': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_refine_in': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, i32, i32, i32, vp]),
    'dcf_op_refine_in_bwd': (i32, [c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_tcn_layer': (i32, [c_f32p] + [c_u8p] + [c_f32p] * 7 + [i32, i32, i32, i64, f32, i32, i32, vp]),
    'dcf_op_tcn_layer_bwd': (i32, [c_f32p] + [c_u8p] + [c_f32p] * 14 + [i32, i32, i32, i64, f32, i32, i32, i32, vp]),
    'dcf_op_sidekick': (i32, [c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
    'dcf_op_gate': (i32, [c_f32p, c_u8p, c_f32p, c_u8p, i32, i32, i32, f64, i32, vp]),
    'dcf_op_encoder': (i32, [vp, ctypes.c_char_p, c_f32p, c_u8p, i32, i32, i32, c_f32p, c_u8p, vp]),
    'dcf_op_enc_pre': (i32, [vp, ctypes.c_char_p, c_f32p, c_u8p, i32, i32, i32, c_f32p, c_f32p, c_f32p, c_f32p, vp]),
    'dcf_op_decoder': (i32, [vp, ctypes.c_char_p, c_f32p, c_u8p, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), vp]),
    'dcf_op_tcn': (i32, [vp, ctypes.c_char_p, c_f32p, c_u8p, i32, i32, i32, i32, c_f32p, vp]),
    'dcf_optim_grad_norm': (i32, [vp, c_i32p, i32, i64, f32, c_f32p, c_f32p, vp]),
    'dcf_optim_scale': (i32, [vp, c_i32p, i32, i64, c_f32p, vp]),
    'dcf_optim_adam_step': (i32, [vp, c_i32p, i32, i64, vp, i32, c_f32p, i32, f32, vp]),
}

# the training extension: dropout and drop-path operators
_DROP = [i32, i32, i32, i32, i64, i32, f32]                 # B, T, C, b0, seed, site, p
TRAIN_SIGNATURES = {
    'dcf_train_ext_version': (i32, []),
    'dcf_op_dropout': (i32, [c_f32p, c_f32p] + _DROP + [vp]),
    'dcf_op_gelu_dropout': (i32, [c_f32p, c_f32p] + _DROP + [vp]),
    'dcf_op_gelu_dropout_bwd': (i32, [c_f32p, c_f32p, c_f32p] + _DROP + [vp]),
    'dcf_op_drop_residual': (i32, [c_f32p, c_u8p, c_f32p, c_u8p, c_f32p, c_f32p] + _DROP + [i32, f32, vp]),
    'dcf_op_drop_residual_bwd': (i32, [c_f32p, c_f32p, c_u8p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p] + _DROP + [i32, f32, i32, vp]),
}


# the data-parallel extension
DIST_SIGNATURES = {
    'dcf_dist_ext_version': (i32, []),
    'dcf_dist_pack_grads': (i32, [vp, c_i32p, i32, i64, f32, vp]),
}


# the attention-gradient extension
ATTN_SIGNATURES = {
    'dcf_attn_ext_version': (i32, []),
    'dcf_op_global_attn_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
}


# the training-front-end extension.  ``nq`` is a HOST array of int32.
FRONT_NO_SKIP = 1             # DCF_FRONT_NO_SKIP
FRONT_SIGNATURES = {
    'dcf_front_ext_version': (i32, []),
    'dcf_op_vidmap_shared': (i32, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_vidmap_shared_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, vp]),
}


# the step-guard extension
GUARD_APPLY, GUARD_SKIP = 0, 1    # DCF_GUARD_APPLY, DCF_GUARD_SKIP


class DcfGuardState(ctypes.Structure):
    """dcf_guard_state: the 48-byte device record of a step guard (``optim.StepGuard`` owns one)"""
    _fields_ = [('verdict', i32), ('first_bad_row', i32), ('n_bad_rows', i32), ('reserved0', i32), ('applied', i64), ('skipped', i64),
                ('last_skipped_attempt', i64), ('conv_flag', i32), ('reserved1', i32)]


GUARD_SIGNATURES = {
    'dcf_guard_ext_version': (i32, []),
    'dcf_guard_grad_norm': (i32, [vp, c_i32p, i32, i64, f32, c_f32p, c_f32p, vp, vp]),
    'dcf_guard_adam_step': (i32, [vp, c_i32p, i32, i64, vp, i32, c_f32p, vp, i32, f32, vp]),
    'dcf_guard_arm': (i32, [vp, vp]),
    'dcf_guard_disarm': (i32, [vp]),
}


# the step-count extension.  ``groups``, ``bc_tables`` and ``bc_len`` are HOST arrays; ``steps`` is int64 in device memory.
CLOCK_MAX_TABLE = 1 << 22     # the longest bias-correction table optim.AdamW(device_count=True) builds
CLOCK_SIGNATURES = {
    'dcf_clock_ext_version': (i32, []),
    'dcf_clock_adam_step': (i32, [vp, c_i32p, i32, i64, vp, i32, vp, c_i32p, c_i64p, c_f32p, vp, i32, f32, vp]),
}


# the half-feature extension.  A half operand is the device address of IEEE binary16 values (``const uint16_t*``); ``text`` /
# ``text_mask`` / ``text_len`` / ``nq_per_video`` are HOST arrays as in SIGNATURES.
c_f16p = ctypes.c_void_p
HALF_SIGNATURES = {
    'dcf_half_ext_version': (i32, []),
    'dcf_forward_eval_h': (i32, [vp, c_f16p, c_f16p, c_u8p, i64, i32, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                 ctypes.POINTER(i32), c_f32p, c_f32p, c_f32p, c_u8p, vp]),
    'dcf_forward_eval_videos_h': (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), i64, ctypes.POINTER(i32),
                                        ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(vp),
                                        c_f32p, c_f32p, c_u8p, vp]),
    'dcf_op_linear_cm_split_h': (i32, [c_f16p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_linear_cm_split_ld_h': (i32, [c_f16p, i64, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_sidekick_h': (i32, [c_f16p, c_f32p, c_f32p, i32, i32, i32, i32, vp]),
}


# the half-feature training-front-end extension.  The operators of FRONT_SIGNATURES with ``vid`` / ``shallow`` the device address of
# IEEE binary16 values; ``nq`` is a HOST array of int32.
FRONT_HALF_SIGNATURES = {
    'dcf_front_half_ext_version': (i32, []),
    'dcf_op_vidmap_shared_h': (i32, [c_f16p, c_f16p, c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, i32, i32, i32, i32, i32, vp]),
    'dcf_op_vidmap_shared_bwd_h': (i32, [c_f16p, c_f16p, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, i32, vp]),
}


# the embedding-stage extension.  ``model`` is a finalized dcf_model.
EMBD_SIGNATURES = {
    'dcf_embd_ext_version': (i32, []),
    'dcf_op_embd_chain': (i32, [vp, c_f32p, i64, c_u8p, i32, i32, i32, c_f32p, c_f32p, i64, vp]),
    'dcf_op_embd_launches': (i32, [vp, c_f32p, i64, c_u8p, i32, i32, i32, c_f32p, c_f32p, i64, vp]),
}


# the batch-assembly extension (include/decafnet_hip_batch.h, csrc/batch.hip).  ``bank`` / ``out`` hold 2- or 4-byte elements; ``desc``
# is int64 in device memory.  The name does not end in the suffix of the registered tables: the record waits in PENDING below.
BATCH_TABLE = {
    'dcf_batch_ext_version': (i32, []),
    'dcf_op_assemble_rows': (i32, [vp, i32, c_i64p, i32, i32, i64, vp, c_u8p, vp]),
}


# The registry: one record per header of include/, all of them exports of the same shared object.  A released table and its header
# are never edited; a new operator family gets a header and a table of its own, a version function that returns 1, and one record at
# the end of this tuple.  lib() binds what the records list, tests/test_abi_headers.py checks every record against its header and the
# built library, and tests/borders.py maps every key to its poisoned-border cases.
Extension = namedtuple('Extension', 'key header version_symbol version version_macro includes table')


def _ext(key, table, includes=('decafnet_hip.h',)):
    return Extension(key, f'decafnet_hip_{key}.h', f'dcf_{key}_ext_version', 1, f'DCF_{key.upper()}_EXT_VERSION', includes, table)


EXTENSIONS = (
    Extension('base', 'decafnet_hip.h', 'dcf_abi_version', 12, None, (), SIGNATURES),
    _ext('train', TRAIN_SIGNATURES),
    _ext('dist', DIST_SIGNATURES),
    _ext('attn', ATTN_SIGNATURES),
    _ext('front', FRONT_SIGNATURES),
    _ext('guard', GUARD_SIGNATURES),
    _ext('clock', CLOCK_SIGNATURES, includes=('decafnet_hip.h', 'decafnet_hip_guard.h')),
    _ext('half', HALF_SIGNATURES),
    _ext('front_half', FRONT_HALF_SIGNATURES),
    _ext('embd', EMBD_SIGNATURES),
)


# Bound by lib() like the records above, but not yet part of the registry: the registry test ties every record of EXTENSIONS to a row
# of tests/borders.TABLE.  The follow-up moves this record to the end of EXTENSIONS together with its ``borders.TABLE`` row (the
# cases are tests/batch_abi_cases.py already, run through the same driver by tests/test_gpu_batch_assemble.py).
PENDING = (
    Extension('batch', 'decafnet_hip_batch.h', 'dcf_batch_ext_version', 1, 'DCF_BATCH_EXT_VERSION', ('decafnet_hip.h',), BATCH_TABLE),
)


# the evaluation-metric extension (include/decafnet_hip_eval.h, csrc/eval_metric.hip).  Every operand is device memory: ``segs`` /
# ``meta`` / ``best`` fp32, ``counts`` / ``ranks`` int32, ``threshs`` float64, ``hits`` / ``n_queries`` int64 and accumulated into.
c_f64p = ctypes.c_void_p
EVAL_TABLE = {
    'dcf_eval_ext_version': (i32, []),
    'dcf_op_recall_update': (i32, [c_f32p, c_i32p, c_f32p, i32, i32, c_i32p, i32, c_f64p, i32, c_i64p, c_i64p, c_f32p, vp]),
}


# Bound by lib() after the records above and waiting for the same follow-up as PENDING: registration at the end of EXTENSIONS
# together with a ``borders.TABLE`` row (the cases are tests/eval_abi_cases.py, run through the same driver by
# tests/test_gpu_eval_metric.py).
STAGED = (
    Extension('eval', 'decafnet_hip_eval.h', 'dcf_eval_ext_version', 1, 'DCF_EVAL_EXT_VERSION', ('decafnet_hip.h',), EVAL_TABLE),
)


# the multi-rank-fit extension (include/decafnet_hip_fit.h, csrc/fit.hip).  ``rows`` fp32, ``offsets`` int64, ``per_video`` / ``out2``
# float64 and ``slot`` fp32 are device memory; ``state`` is the dcf_guard_state of the ARMED guard.
GUARD_REMOTE = 0x100          # DCF_GUARD_REMOTE: the bit of the conv-gradient word that says "raised on some rank"
FIT_TABLE = {
    'dcf_fit_ext_version': (i32, []),
    'dcf_op_loss_table_mean': (i32, [c_f32p, c_i64p, i32, c_f64p, c_f64p, vp]),
    'dcf_guard_word_publish': (i32, [vp, c_f32p, vp]),
    'dcf_guard_word_merge': (i32, [vp, c_f32p, vp]),
}


# Bound by lib() after STAGED and waiting for the same follow-up: registration at the end of EXTENSIONS together with a
# ``borders.TABLE`` row (the cases are tests/fit_abi_cases.py, run through the same driver by tests/test_gpu_loss_table.py).
FIT = (
    Extension('fit', 'decafnet_hip_fit.h', 'dcf_fit_ext_version', 1, 'DCF_FIT_EXT_VERSION', ('decafnet_hip.h', 'decafnet_hip_guard.h'), FIT_TABLE),
)


# the training-log extension (include/decafnet_hip_steplog.h, csrc/steplog.hip).  ``vals`` is a HOST array of device pointers to fp32
# scalars; ``stats`` / ``out`` float64 and ``counts`` int64 are device memory.
STEPLOG_MAX_KEYS = 16         # DCF_STEPLOG_MAX_KEYS
STEPLOG_COLS = 6              # DCF_STEPLOG_COLS
STEPLOG_TABLE = {
    'dcf_steplog_ext_version': (i32, []),
    'dcf_op_steplog_add': (i32, [ctypes.POINTER(vp), i32, c_f64p, c_i64p, vp]),
    'dcf_op_steplog_flush': (i32, [c_f64p, c_i64p, i32, c_f64p, vp]),
}


# Bound by lib() after FIT and waiting for the same follow-up: registration at the end of EXTENSIONS together with a
# ``borders.TABLE`` row (the cases are tests/steplog_abi_cases.py, run through the same driver by tests/test_gpu_steplog.py).
STEPLOG = (
    Extension('steplog', 'decafnet_hip_steplog.h', 'dcf_steplog_ext_version', 1, 'DCF_STEPLOG_EXT_VERSION', ('decafnet_hip.h',), STEPLOG_TABLE),
)


# the attention-map-dropout extension (include/decafnet_hip_attn_drop.h, csrc/attn_drop.hip): the three attention cores -- sliding
# window, global self attention (window = 0 of the local export, with a backward export of its own) and cross attention -- with
# dropout on the map, forward and backward, and channel dropout.  Every operator takes b0, seed, site, p after the arguments of its dropout-free
# form, in the order dcf_op_dropout has them.
_ADROP = [i32, i64, i32, f32]                               # b0, seed, site, p
ATTN_DROP_TABLE = {
    'dcf_attn_drop_ext_version': (i32, []),
    'dcf_op_local_attn_drop': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i32, i32, i32, i32] + _ADROP + [vp]),
    'dcf_op_local_attn_drop_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32] + _ADROP + [vp]),
    'dcf_op_global_attn_drop_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32] + _ADROP + [vp]),
    'dcf_op_xattn_drop': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, i32, i32, i32, i32, i32] + _ADROP + [vp]),
    'dcf_op_xattn_drop_bwd': (i32, [c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32] + _ADROP + [vp]),
    'dcf_op_channel_dropout': (i32, [c_f32p, c_f32p, i32, i32, i32] + _ADROP + [vp]),
}


# Bound by lib() after STEPLOG and waiting for the same follow-up: registration at the end of EXTENSIONS together with a
# ``borders.TABLE`` row (the cases are tests/attn_drop_abi_cases.py, run through the same driver by tests/test_gpu_attn_drop_borders.py).
ATTN_DROP = (
    Extension('attn_drop', 'decafnet_hip_attn_drop.h', 'dcf_attn_drop_ext_version', 1, 'DCF_ATTN_DROP_EXT_VERSION', ('decafnet_hip.h',),
              ATTN_DROP_TABLE),
)


# the selected-clip extension (include/decafnet_hip_select.h, csrc/select.hip; the two forwards in csrc/engine.hip): which clips the
# gates need, the gather that makes clip-major rows of dense features, and the externally gated forward on those rows.  ``clips`` /
# ``pos`` / ``count`` are int32 in device memory; ``text`` / ``text_mask`` / ``text_len`` are HOST arrays as in SIGNATURES.
_FWD_SEL = [i32, c_i32p, vp, c_u8p, i64, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i32), c_f32p, c_f32p, c_f32p, c_u8p, vp]
SELECT_TABLE = {
    'dcf_select_ext_version': (i32, []),
    'dcf_op_select_clips': (i32, [c_f32p, c_u8p, i32, i32, c_i32p, c_i32p, c_i32p, vp]),
    'dcf_op_gather_clip_rows': (i32, [c_f32p, i64, c_i32p, i32, i32, c_f32p, vp]),
    'dcf_op_gather_clip_rows_h': (i32, [c_f16p, i64, c_i32p, i32, i32, c_f16p, vp]),
    'dcf_forward_eval_selected': (i32, [vp, c_f32p] + _FWD_SEL),
    'dcf_forward_eval_selected_h': (i32, [vp, c_f16p] + _FWD_SEL),
}


# Bound by lib() after ATTN_DROP and waiting for the same follow-up: registration at the end of EXTENSIONS together with a
# ``borders.TABLE`` row (the cases are tests/select_abi_cases.py, run through the same driver by tests/test_gpu_select_borders.py).
SELECT = (
    Extension('select', 'decafnet_hip_select.h', 'dcf_select_ext_version', 1, 'DCF_SELECT_EXT_VERSION', ('decafnet_hip.h',), SELECT_TABLE),
)


# selected-clip inference on several videos per forward (include/decafnet_hip_select_videos.h, csrc/select_videos.hip; the two
# forwards in csrc/engine.hip).  ``nq_per_video`` / ``row_first`` and every array of pointers are HOST arrays; ``clips`` / ``pos`` /
# ``counts`` are int32 in device memory.
_PP, _IP = ctypes.POINTER(vp), ctypes.POINTER(i32)
_SELV = [i32, _PP, _PP, i64, _IP, _PP, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p, vp]
_FWD_SELV = [_IP, c_i32p, _PP, _PP, i64, _IP, _PP, _PP, _IP, c_f32p, c_f32p, c_f32p, c_f32p, c_u8p, vp]
SELECT_VIDEOS_TABLE = {
    'dcf_select_videos_ext_version': (i32, []),
    'dcf_op_select_clips_videos': (i32, [c_f32p, c_u8p, i32, i32, _IP, c_i32p, c_i32p, c_i32p, vp]),
    'dcf_op_gather_clip_rows_videos': (i32, [_PP, i64, c_i32p, i32, i32, _IP, i32, c_f32p, vp]),
    'dcf_op_gather_clip_rows_videos_h': (i32, [_PP, i64, c_i32p, i32, i32, _IP, i32, c_f16p, vp]),
    'dcf_select_videos': (i32, [vp] + _SELV),
    'dcf_select_videos_h': (i32, [vp] + _SELV),
    'dcf_forward_eval_videos_selected': (i32, [vp, i32, c_f32p] + _FWD_SELV),
    'dcf_forward_eval_videos_selected_h': (i32, [vp, i32, c_f16p] + _FWD_SELV),
}


# Bound by lib() after SELECT, and waiting for the same follow-up (the cases are tests/select_videos_abi_cases.py, run through the
# border driver by tests/test_gpu_select_videos_borders.py).
SELECT_VIDEOS = (
    Extension('select_videos', 'decafnet_hip_select_videos.h', 'dcf_select_videos_ext_version', 1, 'DCF_SELECT_VIDEOS_EXT_VERSION',
              ('decafnet_hip.h',), SELECT_VIDEOS_TABLE),
)


# selected-clip training (include/decafnet_hip_front_select.h, csrc/front_select.hip): vid_map of the training step and its weight
# gradient on the packed expert rows of the selected clips.  ``row_first`` and ``nq`` are HOST arrays of int32; ``pos`` is int32 in
# device memory; the ``_h`` forms take ``rows`` / ``shallow`` as the device address of IEEE binary16 values.
_FS_FWD = [c_i32p, c_i32p, vp, c_f32p, c_f32p, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, i32, i32, i32, i32, vp]
_FS_BWD = [c_i32p, c_i32p, vp, c_f32p, c_u8p, c_f32p, c_i32p, c_f32p, c_f32p, c_f32p, i32, i32, i32, i32, i32, vp]
FRONT_SELECT_TABLE = {
    'dcf_front_select_ext_version': (i32, []),
    'dcf_op_vidmap_selected': (i32, [c_f32p] + _FS_FWD),
    'dcf_op_vidmap_selected_bwd': (i32, [c_f32p] + _FS_BWD),
    'dcf_op_vidmap_selected_h': (i32, [c_f16p] + _FS_FWD),
    'dcf_op_vidmap_selected_bwd_h': (i32, [c_f16p] + _FS_BWD),
}


# Bound by lib() after SELECT_VIDEOS, and waiting for the same follow-up (the cases are tests/front_select_abi_cases.py, run through
# the border driver by tests/test_gpu_front_select_borders.py).
FRONT_SELECT = (
    Extension('front_select', 'decafnet_hip_front_select.h', 'dcf_front_select_ext_version', 1, 'DCF_FRONT_SELECT_EXT_VERSION',
              ('decafnet_hip.h',), FRONT_SELECT_TABLE),
)


def lib():
    """Load (once) and return the ctypes handle.  torch is imported first so that the HIP runtime
    already mapped by PyTorch-ROCm (same soname, libamdhip64.so.7) is the one this library binds to."""
    global _LIB
    if _LIB is None:
        import torch  # noqa: F401
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f'{SO_PATH} is missing: build it with __graft_entry__.build() '
                               f'(there is no CPU fallback for the grounding path)')
        h = ctypes.CDLL(SO_PATH, mode=ctypes.RTLD_GLOBAL)
        bound = set()
        for ext in EXTENSIONS + PENDING + STAGED + FIT + STEPLOG + ATTN_DROP + SELECT + SELECT_VIDEOS + FRONT_SELECT:
            for name, (res, args) in ext.table.items():
                if name in bound:
                    raise RuntimeError(f'{name} is in two signature tables of _lib.EXTENSIONS / _lib.PENDING / _lib.STAGED / _lib.FIT / '
                                       f'_lib.STEPLOG / _lib.ATTN_DROP / _lib.SELECT / _lib.SELECT_VIDEOS / _lib.FRONT_SELECT')
                bound.add(name)
                fn = getattr(h, name)
                fn.restype = res
                fn.argtypes = args
        _LIB = h
    return _LIB


def check(rc, what=''):
    if rc != 0:
        msg = lib().dcf_last_error().decode(errors='replace')
        raise RuntimeError(f'decafnet_hip {what} failed: {msg}')


def ptr(t):
    """device/host address of a torch tensor (None -> NULL)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
