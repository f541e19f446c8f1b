"""ctypes binding of csrc/libafr.so (C ABI declared in include/afr.h).

There is no fallback: if the shared library is missing or does not export every symbol the header
declares, importing this module raises.  `python -c "import __graft_entry__ as g; g.build()"` (or
csrc/build.sh) builds it in-tree for gfx950.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AFR_LIB_PATH") or os.path.join(HERE, "csrc", "libafr.so")   # override: kernel A/B experiments

AFR_KIND_SHEET, AFR_KIND_GLYPH, AFR_KIND_PIXEL = 0, 1, 2
AFR_F32, AFR_BF16, AFR_BF16X3 = 0, 1, 2
AFR_TARGET_U8, AFR_TARGET_F32 = 0, 1
AFR_LOSS_MSE, AFR_LOSS_BCE = 0, 1
LOSS_KINDS = {"mse": AFR_LOSS_MSE, "bce": AFR_LOSS_BCE}
AFR_OPT_ADAMW, AFR_OPT_LION = 0, 1
OPT_KINDS = {"adamw": AFR_OPT_ADAMW, "lion": AFR_OPT_LION}
STAT_KINDS = {"params": 0, "grads": 1, "exp_avg": 2, "exp_avg_sq": 3, "ema": 4}      # AFR_STAT_*: the buffer afr_tensor_stats reads

AFR_OK, AFR_EINVAL, AFR_ESTATE, AFR_EHIP, AFR_EUNSUPPORTED = 0, -1, -2, -3, -4

AFR_MAX_HIDDEN = 8
BUF_U, BUF_Z, BUF_DZ, BUF_W1T, BUF_W2T, BUF_ACT = 0, 1, 2, 4, 5, 16
GEMM_BIAS, GEMM_RELU, GEMM_RELU_MASK, GEMM_OUT_BF16, GEMM_A_KSTRIDED, GEMM_B_KSTRIDED = 1, 2, 4, 8, 16, 32


def loss_kind(loss):
    """"mse" | "bce" -> AFR_LOSS_*; anything else is a ValueError."""
    if not isinstance(loss, str) or loss not in LOSS_KINDS:
        raise ValueError(f"loss must be 'mse' or 'bce', got {loss!r}")
    return LOSS_KINDS[loss]


def opt_kind(optimizer):
    """"adamw" | "lion" -> AFR_OPT_*; anything else is a ValueError."""
    if not isinstance(optimizer, str) or optimizer not in OPT_KINDS:
        raise ValueError(f"optimizer must be 'adamw' or 'lion', got {optimizer!r}")
    return OPT_KINDS[optimizer]


class AfrConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("dtype", C.c_int32), ("max_batch", C.c_int32), ("vocab", C.c_int32),
        ("embed_dim", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
        ("max_length", C.c_int32), ("heads", C.c_int32), ("fc_dim", C.c_int32),
        ("p_embed", C.c_float), ("p_attn", C.c_float), ("p_fc", C.c_float), ("ln_eps", C.c_float),
        ("n_hidden", C.c_int32), ("hidden", C.c_int32 * AFR_MAX_HIDDEN), ("n_fonts", C.c_int32),
        ("seed", C.c_uint64), ("rank", C.c_int32), ("reserved", C.c_int32),
        ("loss", C.c_int32),
    ]


class AfrOptRange(C.Structure):
    """One merged range of the optimizer groups (include/afr.h afr_opt_range): flat elements up to `end` take these multipliers."""
    _fields_ = [("end", C.c_int64), ("lr_mult", C.c_float), ("wd_mult", C.c_float)]


class AfrTensorSeg(C.Structure):
    """One tensor of afr_op_tensor_stats' host table (include/afr.h afr_tensor_seg): numel elements from element off (a multiple of 4)."""
    _fields_ = [("off", C.c_int64), ("numel", C.c_int64)]


class AfrSheetParams(C.Structure):
    """The ten small tensors of the sheet front end (include/afr.h afr_sheet_params), device pointers."""
    _fields_ = [(n, C.c_void_p) for n in ("pos", "emb", "w_in", "b_in", "w_o", "b_o", "ln_g", "ln_b", "w1", "b1")]


class AfrSheetDropout(C.Structure):
    """One training pass's dropout description (include/afr.h afr_sheet_dropout)."""
    _fields_ = [("seed", C.c_uint64), ("step", C.c_uint64), ("rank", C.c_int32), ("p_embed", C.c_float), ("p_attn", C.c_float),
                ("p_fc", C.c_float)]


class AfrSheetSlabLayout(C.Structure):
    """Offsets in floats of the ten tensors inside one partial-gradient slab, and the slab's length (afr_sheet_slab_layout)."""
    _fields_ = [(n, C.c_int32) for n in ("pos", "emb", "w_in", "b_in", "w_o", "b_o", "ln_g", "ln_b", "w1", "b1", "total")]


class AfrGlyph1Layout(C.Structure):
    """Offsets in floats of the six tensors inside one slab of the fused glyph step, and the slab's length (afr_glyph1_layout)."""
    _fields_ = [(n, C.c_int32) for n in ("emb", "font", "w1", "b1", "w2", "b2", "total")]


LIN_FWD, LIN_DX, LIN_DW, LIN_PAIR = 0, 1, 2, 3      # AFR_LIN_*: which product of a Linear afr_op_linear issues


class AfrLinearTail(C.Structure):
    """The step-only tails of one Linear product (include/afr.h afr_linear_tail); pointers are device pointers."""
    _fields_ = [("ld_out", C.c_int32), ("ldx", C.c_int32), ("ldaux", C.c_int32), ("ld_db", C.c_int32),
                ("target", C.c_void_p), ("target_rows", C.c_void_p), ("target_dtype", C.c_int32), ("loss_kind", C.c_int32),
                ("mean_elems", C.c_int64), ("loss_accum", C.c_void_p), ("loss_scratch", C.c_void_p),
                ("mask_out", C.c_void_p), ("x_rows", C.c_void_p),
                ("aux", C.c_void_p), ("aux_rows", C.c_void_p), ("mask_in", C.c_void_p), ("ldmask", C.c_int32),
                ("splitk", C.c_int32), ("db", C.c_void_p), ("opt_kind", C.c_int32), ("reserved", C.c_int32),
                ("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("shadow", C.c_void_p),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("grad_scale", C.c_float), ("t", C.c_int64)]


class AfrReduceStep(C.Structure):
    """The fused optimizer step of one grouped reduce (include/afr.h afr_reduce_step): gbase, p, m, v, shadow are device pointers;
    lr_mult, wd_mult, shT, tN, tK host arrays with one entry per segment, or NULL."""
    _fields_ = [("opt_kind", C.c_int32), ("reserved", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("reserved2", C.c_float), ("t", C.c_int64),
                ("gbase", C.c_void_p), ("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("shadow", C.c_void_p),
                ("lr_mult", C.POINTER(C.c_float)), ("wd_mult", C.POINTER(C.c_float)),
                ("shT", C.POINTER(C.c_void_p)), ("tN", C.POINTER(C.c_int32)), ("tK", C.POINTER(C.c_int32))]


class AfrGlyphAtlas(C.Structure):
    """The glyph atlas afr_op_compose_sheets blits from (include/afr.h afr_glyph_atlas); pointers are device pointers."""
    _fields_ = [("cells", C.c_void_p), ("adv64", C.c_void_p), ("kern64", C.c_void_p), ("n_codes", C.c_int32), ("cell_h", C.c_int32),
                ("cell_w", C.c_int32), ("origin_x", C.c_int32), ("origin_y", C.c_int32)]


class AfrSheetGeometry(C.Structure):
    """Sheet size, wrap width in 1/64 px and the baselines of the lines that are drawn (include/afr.h afr_sheet_geometry)."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("wrap_width64", C.c_int32), ("n_lines", C.c_int32), ("baseline", C.c_int32 * 16)]


_vp, _i32, _i64, _f32, _u64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_size_t

# name -> (restype, argtypes): every function include/afr.h declares
SIGNATURES = {
    "afr_version": (_i32, []),
    "afr_last_error": (C.c_char_p, []),
    "afr_plan_create": (_i32, [C.POINTER(AfrConfig), C.POINTER(_vp)]),
    "afr_plan_destroy": (_i32, [_vp]),
    "afr_param_elems": (_i64, [_vp]),
    "afr_param_count": (_i32, [_vp]),
    "afr_param_info": (_i32, [_vp, _i32, C.c_char_p, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_int32), C.POINTER(_i64)]),
    "afr_workspace_bytes": (_sz, [_vp]),
    "afr_bind": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "afr_sync_params": (_i32, [_vp, _vp]),
    "afr_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _u64, _vp]),
    "afr_loss_grad": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp]),
    "afr_set_output_grad": (_i32, [_vp, _vp, _i32, _vp]),
    "afr_backward": (_i32, [_vp, _vp]),
    "afr_backward_stages": (_i32, [_vp]),
    "afr_backward_stage": (_i32, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "afr_forward_loss": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _u64, _vp]),
    "afr_adamw_step": (_i32, [_vp, _f32, _f32, _f32, _f32, _f32, _i64, _f32, _vp]),
    "afr_set_grad_clip": (_i32, [_vp, _f32, _vp]),
    "afr_set_optimizer": (_i32, [_vp, _i32]),
    "afr_set_param_groups": (_i32, [_vp, C.POINTER(_f32), C.POINTER(_f32), _i32]),
    "afr_param_group_ranges": (_i32, [_vp, C.POINTER(AfrOptRange), _i32]),
    "afr_grad_sumsq": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "afr_set_ema": (_i32, [_vp, _vp, _f32, _i32]),
    "afr_ema_update": (_i32, [_vp, _vp, _vp]),
    "afr_op_ema": (_i32, [_vp, _vp, _i64, _f32, _vp, _vp]),
    "afr_use_ema": (_i32, [_vp, _i32, _vp]),
    "afr_train_step": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _u64, _i32, _f32, _f32, _f32, _f32, _f32, _i64, _vp]),
    "afr_bind_dataset": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i32]),
    "afr_forward_rows": (_i32, [_vp, _vp, _i32, _vp, _i32, _u64, _vp]),
    "afr_loss_grad_rows": (_i32, [_vp, _vp, _i32, _i64, _vp, _vp]),
    "afr_forward_loss_rows": (_i32, [_vp, _vp, _i32, _i64, _vp, _u64, _vp]),
    "afr_train_step_rows": (_i32, [_vp, _vp, _i32, _i64, _vp, _u64, _i32, _f32, _f32, _f32, _f32, _f32, _i64, _vp]),
    "afr_eval": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "afr_eval_rows": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "afr_tensor_stats_chunk": (_i32, []),
    "afr_tensor_stats": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "afr_error_flags": (_i32, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "afr_profile_dominant": (_i32, [_vp, _i32]),
    "afr_profile_read": (_i32, [_vp, C.c_char_p, _i32, C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "afr_profile_dump": (_i32, [_vp, C.c_char_p, _i32]),
    "afr_debug_copy": (_i32, [_vp, _i32, _vp, _sz, C.POINTER(_sz), _vp]),
    "afr_debug_sheet_gather": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "afr_op_gemm": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "afr_op_gemm_fix_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "afr_op_gemm_fix": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "afr_op_gemm_pair_plan": (_i32, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_sz)]),
    "afr_op_gemm_pair": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "afr_op_linear_pair_plan": (_i32, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_sz)]),
    "afr_op_linear": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.POINTER(AfrLinearTail), _vp, _sz, C.c_char_p, _i32, _vp]),
    "afr_plan_pair_chain": (_i32, [_vp, _i32, _i32]),
    "afr_op_linear_chain_plan": (_i32, [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_sz)]),
    "afr_op_linear_chain_block": (_i32, [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "afr_op_linear_chain": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(AfrLinearTail), _vp, _vp, _vp, _vp, C.POINTER(AfrLinearTail),
                                   _i32, _i32, _i32, _i32, _vp, _sz, C.c_char_p, _i32, _vp]),
    "afr_op_linear_chain_l1_plan": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_sz)]),
    "afr_op_linear_chain_l1_block": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                            C.POINTER(_i32)]),
    "afr_op_linear_chain_l1": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(AfrLinearTail), _vp, _vp, _vp, _vp, C.POINTER(AfrLinearTail),
                                      _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp,
                                      _vp, _i32, _i32, _f32, _vp, C.c_char_p, _i32, _vp]),
    "afr_op_reduce": (_i32, [_vp, _vp, _i32, _i64, _i64, _f32, _i32, _vp]),
    "afr_op_reduce_group": (_i32, [_i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "afr_op_reduce_group_step": (_i32, [_i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64),
                                        C.POINTER(AfrReduceStep), C.c_char_p, _i32, _vp]),
    "afr_op_adamw": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i64, _f32, _vp]),
    "afr_op_adamw_clip": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i64, _f32, _vp, _f32, _vp]),
    "afr_op_lion": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _vp, _f32, _vp]),
    "afr_op_opt_groups": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, C.POINTER(AfrOptRange), _i32, _f32, _f32, _f32, _f32, _f32, _i64, _f32,
                                 _vp, _f32, _vp]),
    "afr_op_mse_grad": (_i32, [_i32, _vp, _vp, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "afr_op_bce_grad": (_i32, [_i32, _vp, _vp, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "afr_op_eval": (_i32, [_i32, _i32, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "afr_op_tensor_stats_scratch_bytes": (_sz, [C.POINTER(AfrTensorSeg), _i32]),
    "afr_op_tensor_stats": (_i32, [_vp, _vp, C.POINTER(AfrTensorSeg), _i32, _vp, _vp, _sz, _vp]),
    "afr_op_f32_to_bf16": (_i32, [_vp, _vp, _i64, _vp]),
    "afr_op_dataset_text": (_i32, [_i64, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp]),
    "afr_op_dataset_text_w": (_i32, [_i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "afr_op_text_weights": (_i32, [_vp, _i32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "afr_op_dataset_text_m": (_i32, [_i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "afr_op_pair_errors": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp, _vp]),
    "afr_op_pair_weights": (_i32, [_vp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "afr_op_compose_sheets": (_i32, [C.POINTER(AfrGlyphAtlas), C.POINTER(AfrSheetGeometry), _vp, _i32, _vp, _i64, _vp, _vp, _vp]),
    "afr_op_sheet_char_errors": (_i32, [C.POINTER(AfrGlyphAtlas), C.POINTER(AfrSheetGeometry), _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "afr_op_sheet_read_back": (_i32, [C.POINTER(AfrGlyphAtlas), C.POINTER(AfrSheetGeometry), _vp, _i32, _vp, _i64, _vp, C.POINTER(C.c_uint32),
                                      _vp, _vp, _vp, _vp, _vp]),
    "afr_op_f32_to_fp8": (_i32, [_vp, _vp, _i64, _f32, _vp]),
    "afr_op_gemm_fp8": (_i32, [_i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "afr_pixel_bwd_blocks": (_i32, [C.c_longlong]),
    "afr_pixel_attn_chunk": (_i32, [_i32]),
    "afr_op_pixel_ctx": (_i32, [_i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "afr_op_pixel_ctx_bwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "afr_op_pixel_add_ln": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _vp]),
    "afr_op_pixel_attn": (_i32, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "afr_op_pixel_attn_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "afr_op_pixel_head": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "afr_op_pixel_head_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "afr_op_pixel_ln_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "afr_sheet_blocks": (_i32, [_i32]),
    "afr_sheet_save_floats": (_sz, [_i32, _i32]),
    "afr_op_sheet_fwd": (_i32, [_i32, C.POINTER(AfrSheetParams), _vp, _i32, _i32, _i32, _i32, _i32, _f32, C.POINTER(AfrSheetDropout), _vp, _vp, _vp, _vp]),
    "afr_op_sheet_bwd": (_i32, [_i32, C.POINTER(AfrSheetParams), _vp, _i32, _i32, _i32, _i32, _i32, _f32, C.POINTER(AfrSheetDropout), _vp, _vp, _vp,
                                C.POINTER(AfrSheetSlabLayout), _vp]),
    "afr_glyph_k0": (_i32, [_i32, _i32, _i32]),
    "afr_glyph_l1_bwd_blocks": (_i32, [_i32]),
    "afr_embed_bwd_blocks": (_i32, [_i32]),
    "afr_glyph_l1_bwd_fused_eligible": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "afr_glyph_l1_bwd_fused_split": (_i32, [_i32, _i32]),
    "afr_glyph_l1_bwd_fused_blocks": (_i32, [_i32, _i32]),
    "afr_glyph_l1_bwd_fused_slab_floats": (C.c_longlong, [_i32, _i32, _i32, _i32]),
    "afr_op_glyph_embed": (_i32, [_i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "afr_op_glyph_combo": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "afr_op_glyph_l1_bwd": (_i32, [_vp, _i32, C.c_longlong, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "afr_op_glyph_l1_bwd_fused": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "afr_op_glyph_embed_bwd": (_i32, [_i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "afr_op_glyph_l1_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "afr_glyph1_rows": (_i32, [_i32]),
    "afr_glyph1_colsplit": (_i32, [_i32, _i32, _i32]),
    "afr_glyph1_blocks": (_i32, [_i32, _i32, _i32]),
    "afr_glyph1_eligible": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "afr_op_glyph1_step": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                  _i64, _vp, C.POINTER(AfrGlyph1Layout), _vp, _vp, _vp, _vp]),
    "afr_op_transpose_bf16": (_i32, [_vp, _vp, _i32, _i32, _vp]),
}


class AfrError(RuntimeError):
    """code: the AFR_E* value of a failed library call (None when the Python side raised it without one)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension is the only implementation of the hot path "
            "(no CPU fallback).  Build it with ai-font-renderer_amd/csrc/build.sh or __graft_entry__.build().")
    # torch first: it ships its own libamdhip64, and libafr.so must bind to THAT runtime instance (the device pointers
    # it is handed come from torch's allocator).  Loaded before torch, libafr.so would pull in /opt/rocm's copy and the
    # process would hold two HIP runtimes ("no ROCm-capable device is detected" at the first launch).
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load()
    return _lib


def check(rc):
    if rc != 0:
        raise AfrError(f"libafr error {rc}: {lib().afr_last_error().decode()}", rc)
