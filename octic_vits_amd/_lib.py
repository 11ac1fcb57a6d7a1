"""ctypes binding of liboctic_hip.so (the C ABI declared in include/octic_hip.h).

There is NO fallback: if the HIP library is missing or a symbol is absent, importing the ops fails
loudly.  Nothing in this package routes through a CPU or composite-torch implementation of a hot op.
"""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCTIC_LIB") or os.path.join(HERE, "liboctic_hip.so")   # OCTIC_LIB: developer A/B builds
HEADER_PATH = os.path.join(HERE, "..", "include", "octic_hip.h")

F32, BF16, U8 = 0, 1, 2
ABI_VERSION = 20
# knobs of octic_route_override (include/octic_hip.h)
(ROUTE_DENSE_TILE, ROUTE_DENSE_SPLIT, ROUTE_WGRAD_SLABS, ROUTE_WGRAD_TILE, ROUTE_LINEAR_RING, ROUTE_RING_EVEN,
 ROUTE_ATTN_LEGACY, ROUTE_ATTN_ONLINE, ROUTE_ATTN_BWD_PAIR, ROUTE_DENSE_IMAGE, ROUTE_DENSE_CLS2, ROUTE_ATTN_STREAM) = range(12)

# ROUTE_DENSE_TILE, added to the width (0 | 4 | 5): what octic_dense_gemm_nt_tokens_adaptive chooses (0 = by its rule)
DENSE_ADAPT_WIDE, DENSE_ADAPT_NARROW = 16, 32
# ROUTE_DENSE_IMAGE, added to its value (0 .. 3): what octic_dense_gemm_nt_tokens_image does (0 = by its model)
DENSE_IMAGE_ALWAYS, DENSE_IMAGE_CLS_APART, DENSE_IMAGE_NEVER = 4, 8, 16

# kernel ids of octic_attn_plan (include/octic_hip.h)
(ATTN_FWD_PERSIST, ATTN_FWD_A80_ONESHOT, ATTN_FWD_A80_ONLINE, ATTN_FWD_RESIDENT, ATTN_FWD_STREAM, ATTN_FWD_F32) = range(6)
ATTN_BWD_SINGLE, ATTN_BWD_PAIR, ATTN_BWD_STREAM, ATTN_BWD_F32 = range(4)
# kernel ids of octic_linear_d8_plan and octic_linear_d8_wgrad_plan
LINEAR_WREG, LINEAR_RING, LINEAR_CLASSIC = range(3)
WGRAD_RING, WGRAD_TILED = range(2)
# op of octic_dense_f32_plan / octic_dense_f32_workspace_bytes
DENSE_F32_NT, DENSE_F32_NN, DENSE_F32_TN = range(3)

c_i64, c_int, c_float, c_void_p = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
c_double = ctypes.c_double


class OcticView(ctypes.Structure):
    _fields_ = [("ptr", c_void_p * 5), ("ld", c_i64 * 5)]


PtrArray5 = c_void_p * 5
PtrArray4, I64Array4 = c_void_p * 4, c_i64 * 4     # the per-layer operand tables of octic_depth_logits
VP = ctypes.POINTER(OcticView)

# name -> (restype, argtypes)
_PROTOS = {
    "octic_abi_version": (c_int, []),
    "octic_strerror": (ctypes.c_char_p, [c_int]),
    "octic_route_override": (c_int, [c_int, c_int]),
    "octic_gelu_d8_fwd": (c_int, [VP, VP, c_i64, c_int, c_int, c_void_p]),
    "octic_gelu_d8_bwd": (c_int, [VP, VP, VP, c_i64, c_int, c_int, c_void_p]),
    "octic_gelu_d8_fwd_skip": (c_int, [VP, VP, c_i64, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_gelu_d8_bwd_skip": (c_int, [VP, VP, VP, c_i64, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_layernorm_d8_fwd": (c_int, [VP, VP, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_float, c_int, c_void_p]),
    "octic_layernorm_d8_bwd_blocks": (c_int, [c_i64]),
    "octic_layernorm_d8_bwd": (c_int, [VP, VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "octic_layernorm_d8_bwd_cast": (c_int, [VP, VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_int, c_void_p, c_i64,
                                            c_void_p, c_void_p]),
    "octic_layernorm_d8_bwd_skip": (c_int, [VP, VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_int, c_int, c_void_p, c_i64,
                                            c_void_p]),
    "octic_layernorm_d8_bwd_cast_skip": (c_int, [VP, VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_int, c_void_p, c_i64,
                                                 c_void_p, c_void_p, c_i64, c_void_p]),
    "octic_layernorm_d8_bwd_cast_inplace": (c_int, [VP, VP, c_void_p, c_void_p, VP, c_void_p, c_i64, c_int, c_void_p, c_i64,
                                                    c_void_p, c_void_p, c_i64, c_void_p]),
    "octic_layernorm_d8_bwd_finish": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octic_layernorm_d8_bwd_finish_batch": (c_int, [c_void_p, c_int, c_void_p]),
    "octic_sample_blocks": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_void_p]),
    "octic_linear_d8_fwd": (c_int, [VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int,
                                    c_int, c_int, c_void_p]),
    "octic_linear_d8_fwd_skip": (c_int, [VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int,
                                         c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_linear_d8_fwd_dropped": (c_int, [VP, c_void_p, c_void_p, VP, VP, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int,
                                            c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_linear_d8_tile_n": (c_int, [c_i64, c_int, c_int]),
    "octic_linear_d8_plan": (c_int, [c_i64, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_linear_d8_ring_order": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "octic_linear_d8_ring_order_dropped": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p]),
    "octic_linear_d8_wgrad_tile": (c_int, [c_i64, c_int, c_int]),
    "octic_linear_d8_wgrad_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_linear_d8_wgrad_splits": (c_int, [c_i64, c_int, c_int]),
    "octic_linear_d8_wgrad": (c_int, [VP, VP, c_i64, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "octic_linear_d8_wgrad_skip": (c_int, [VP, VP, c_i64, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "octic_linear_d8_wgrad_order_dropped": (c_int, [c_i64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                                    c_void_p, c_void_p]),
    "octic_linear_d8_wgrad_finish": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_linear_d8_wgrad_finish_batch": (c_int, [c_void_p, c_int, c_void_p]),
    "octic_linear_d8_wgrad_has_colsum": (c_int, [c_int, c_int, c_int]),
    "octic_linear_d8_wgrad_plan": (c_int, [c_i64, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_lamb_workspace_floats": (c_i64, [c_int, c_int]),
    "octic_lamb_step": (c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_float, c_float, c_float, c_float, c_float,
                                                  c_int, c_float, c_void_p, c_void_p]),
    "octic_adamw_step": (c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_float, c_float, c_float, c_float, c_float,
                                                   c_int, c_float, c_void_p, c_void_p]),
    "octic_lamb_step_hp": (c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                                     c_int, c_void_p, c_void_p, c_void_p]),
    "octic_adamw_step_hp": (c_int, [c_void_p] * 10 + [c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                                      c_int, c_void_p, c_void_p, c_void_p]),
    "octic_dense_blocks": (c_int, [c_i64]),
    "octic_dense_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                          c_float, c_void_p]),
    "octic_dense_resid_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_int,
                                                c_void_p, c_void_p, c_void_p, c_i64, c_int, c_float, c_void_p]),
    "octic_dense_resid_layernorm_fwd_skip": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p,
                                                     c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_float, c_void_p]),
    "octic_dense_layernorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_i64, c_int, c_void_p]),
    "octic_dense_layernorm_bwd_tail": (c_int, [c_void_p] * 10 + [c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "octic_dense_layernorm_bwd_tail_skip": (c_int, [c_void_p] * 10 + [c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p, c_i64,
                                                                      c_void_p]),
    "octic_dense_layernorm_bwd_tail_inplace": (c_int, [c_void_p] * 9 + [c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p, c_i64,
                                                                        c_void_p]),
    "octic_dense_finish": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_dense_finish_batch": (c_int, [c_void_p, c_int, c_void_p]),
    "octic_dense_gelu_blocks": (c_int, []),
    "octic_dense_gelu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "octic_swiglu_blocks": (c_int, []),
    "octic_swiglu_fwd": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64, c_int, c_void_p]),
    "octic_swiglu_bwd": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p]),
    "octic_dense_layernorm_fwd_rows": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_float,
                                               c_void_p, c_void_p, c_void_p]),
    "octic_dense_layernorm_bwd_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                               c_int, c_void_p, c_void_p]),
    "octic_scale_residual_fwd_rows": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int,
                                              c_void_p, c_void_p]),
    "octic_scale_residual_bwd_rows": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i64,
                                              c_int, c_void_p, c_void_p]),
    "octic_softmax_center": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_float, c_void_p, c_i64, c_int, c_void_p]),
    "octic_soft_ce_fwd": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                  c_void_p]),
    "octic_soft_ce_bwd": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                  c_i64, c_int, c_void_p]),
    "octic_sinkhorn_slabs": (c_int, [c_i64]),
    "octic_sinkhorn_protos": (c_int, [c_void_p, c_int, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int,
                                      c_void_p]),
    "octic_sinkhorn_rows": (c_int, [c_void_p, c_int, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "octic_sinkhorn_final": (c_int, [c_void_p, c_int, c_i64, c_float, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "octic_koleo_ok": (c_int, [c_i64, c_i64, c_i64]),
    "octic_koleo_fwd": (c_int, [c_void_p, c_int, c_i64, c_i64, c_i64, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "octic_koleo_bwd": (c_int, [c_void_p, c_int, c_i64, c_i64, c_i64, c_i64, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_i64, c_void_p]),
    "octic_head_rows": (c_int, [c_void_p, c_int, c_i64, c_i64, c_int, c_void_p, c_i64, c_int, c_void_p]),
    "octic_l2norm_ok": (c_int, [c_i64, c_i64]),
    "octic_l2norm_rows_fwd": (c_int, [c_void_p, c_int, c_i64, c_i64, c_i64, c_float, c_void_p, c_int, c_i64, c_void_p, c_void_p]),
    "octic_l2norm_rows_bwd": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_int, c_i64, c_void_p, c_i64, c_i64, c_float, c_void_p,
                                      c_i64, c_void_p]),
    "octic_weight_norm_prep": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_weight_norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
    "octic_scale_residual_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int,
                                         c_void_p]),
    "octic_scale_residual_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p,
                                         c_i64, c_int, c_void_p]),
    "octic_colsum_blocks": (c_int, [c_i64]),
    "octic_colsum_a1": (c_int, [VP, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "octic_cast_rowscale": (c_int, [VP, VP, c_void_p, c_i64, c_i64, c_int, c_int, c_void_p]),
    "octic_linear_d8_prep": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "octic_linear_d8_prep_batch_blocks": (c_int, [c_int, c_int]),
    "octic_linear_d8_prep_batch": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "octic_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int,
                               c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_float, c_void_p]),
    "octic_attn_fwd_packed": (c_int, [c_void_p] * 3 + [c_i64, c_int, c_int, c_int, c_i64, c_i64, c_float, c_void_p]),
    "octic_attn_bwd_packed": (c_int, [c_void_p] * 6 + [c_i64, c_int, c_int, c_int, c_i64, c_i64, c_i64, c_float, c_int, c_void_p]),
    "octic_attn_bwd": (c_int, [c_void_p] * 10 + [c_i64, c_int, c_int, c_int] + [c_i64] * 9 + [c_float, c_int, c_void_p]),
    # the four above with sample_scale (nullable [B] f32: 0 = the sample's branch is dropped) in front of the stream
    "octic_attn_fwd_skip": (c_int, [c_void_p] * 5 + [c_i64, c_int, c_int, c_int] + [c_i64] * 6 + [c_float, c_void_p, c_void_p]),
    "octic_attn_bwd_skip": (c_int, [c_void_p] * 10 + [c_i64, c_int, c_int, c_int] + [c_i64] * 9 + [c_float, c_int, c_void_p, c_void_p]),
    "octic_attn_fwd_packed_skip": (c_int, [c_void_p] * 3 + [c_i64, c_int, c_int, c_int, c_i64, c_i64, c_float, c_void_p, c_void_p]),
    "octic_attn_bwd_packed_skip": (c_int, [c_void_p] * 6 + [c_i64, c_int, c_int, c_int, c_i64, c_i64, c_i64, c_float, c_int, c_void_p, c_void_p]),
    "octic_attn_fwd_f32": (c_int, [c_void_p] * 5 + [c_i64, c_int, c_int, c_int] + [c_i64] * 6 + [c_float, c_void_p]),
    "octic_attn_bwd_f32": (c_int, [c_void_p] * 10 + [c_i64, c_int, c_int, c_int] + [c_i64] * 9 + [c_float, c_int, c_void_p]),
    "octic_attn_plan": (c_int, [c_int, c_int, c_int, c_i64, c_i64, c_i64, ctypes.POINTER(c_int)]),
    "octic_attn_skip_plan": (c_int, [c_int, c_int, c_int, c_i64, c_i64, c_i64, ctypes.POINTER(c_int)]),
    "octic_attn_pack_heads": (c_int, [VP, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p]),
    "octic_attn_unpack_heads": (c_int, [c_void_p, VP, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p]),
    "octic_handoff_cat_fwd": (c_int, [VP, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "octic_handoff_cat_bwd": (c_int, [c_void_p, VP, c_i64, c_int, c_void_p]),
    "octic_power_spectrum_fwd": (c_int, [VP, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "octic_power_spectrum_bwd": (c_int, [c_void_p, VP, VP, c_i64, c_int, c_void_p]),
    "octic_im2col_patches": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "octic_lift_gemm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_int,
                                c_int, c_void_p]),
    "octic_lift_wgrad_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_lift_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int, c_int, c_int, c_void_p]),
    "octic_dense_prep_batch_blocks": (c_int, [c_int, c_int]),
    "octic_dense_prep_batch": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "octic_dense_gemm_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_dense_gemm_colsum_rows": (c_int, [c_int, c_int, c_int]),
    "octic_dense_gemm_tile": (c_int, [c_int, c_int, c_int, c_int]),
    "octic_dense_gemm_nt": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p, c_void_p, c_i64,
                                    c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "octic_dense_gemm_nt_tokens": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p, c_void_p,
                                           c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_void_p]),
    "octic_dense_gemm_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_dense_gemm_nt_tokens_skip": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p, c_void_p,
                                                c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "octic_dense_gemm_plan_dropped": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_dense_gemm_order_dropped": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "octic_dense_gemm_nt_tokens_adaptive": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p, c_void_p,
                                                    c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "octic_dense_gemm_plan_adaptive": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_dense_gemm_order_adaptive": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                c_void_p, c_void_p]),
    "octic_dense_gemm_nt_tokens_adaptive_cls": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p,
                                                        c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p,
                                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "octic_dense_gemm_plan_adaptive_cls": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_dense_gemm_order_adaptive_cls": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "octic_dense_gemm_nt_tokens_image": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_int, c_void_p,
                                                 c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_double, c_void_p]),
    "octic_dense_gemm_plan_image": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, ctypes.POINTER(c_int)]),
    "octic_dense_gemm_order_image": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_double, c_int, c_void_p, c_void_p,
                                             c_void_p, c_int, c_void_p, c_void_p]),
    "octic_dense_colsum": (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_void_p]),
    "octic_dense_colsum_skip": (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_void_p, c_i64, c_void_p]),
    "octic_dense_wgrad_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_dense_wgrad_tile": (c_int, [c_int, c_int, c_int]),
    "octic_dense_wgrad_plan": (c_int, [c_int, c_int, c_int, c_int, c_i64, ctypes.POINTER(c_int)]),
    "octic_dense_wgrad_tn": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
    "octic_dense_wgrad_pair_workspace_bytes": (c_i64, [c_int, c_int, c_int, c_int]),
    "octic_dense_wgrad_tn_pair": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_i64,
                                          c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "octic_dense_wgrad_tn_skip": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p]),
    "octic_dense_wgrad_tn_pair_skip": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_i64,
                                               c_i64, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "octic_dense_f32_plan": (c_int, [c_int, c_i64, c_i64, c_i64, c_i64, ctypes.POINTER(c_int)]),
    "octic_dense_f32_workspace_bytes": (c_i64, [c_int, c_i64, c_i64, c_i64]),
    "octic_dense_f32_nt": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_i64, c_int,
                                   c_void_p, c_i64, c_void_p]),
    "octic_dense_f32_nn": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p]),
    "octic_dense_f32_tn": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p,
                                   c_i64, c_void_p]),
    "octic_dense_gelu_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "octic_probe_features": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_i64, c_i64, c_int, c_i64, c_int, c_int, c_void_p,
                                     c_i64, c_void_p]),
    "octic_probe_forward": (c_int, [c_void_p, c_int, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p]),
    "octic_probe_ce": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "octic_probe_sgd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p, c_float, c_void_p]),
    "octic_attnpool_fold": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_attnpool_softmax": (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_void_p]),
    "octic_attnpool_pool": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_attnpool_value": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "octic_attnpool_dinput": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_i64, c_void_p]),
    "octic_attnpool_dweight": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_float, c_void_p,
                                       c_void_p]),
    "octic_attnpool_colsum": (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "octic_attnpool_dz": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_attnpool_dwv": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_attnpool_dscores": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_attnpool_unfold": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_seg_ldd": (c_int, [c_int]),
    "octic_seg_slabs": (c_int, [c_i64, c_int, c_int]),
    "octic_seg_workspace_bytes": (c_i64, [c_i64, c_int, c_int]),
    "octic_seg_value_dlogits": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "octic_seg_predict": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "octic_seg_wgrad": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_int, c_void_p, c_double, c_double, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "octic_seg_colstats_workspace_bytes": (c_i64, [c_i64, c_int]),
    "octic_seg_colstats": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_seg_standardize": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    "octic_seg_patch_mode": (c_int, [c_void_p, c_int, c_i64, c_int, c_void_p, c_void_p]),
    "octic_seg_confusion": (c_int, [c_void_p, c_int, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_seg_knn_plan": (c_int, [c_i64, c_i64, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_seg_knn_workspace_bytes": (c_i64, [c_i64, c_i64, c_int, c_int, c_int, c_int]),
    "octic_seg_rownorms": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p]),
    "octic_seg_knn": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "octic_seg_rownorms_bf16": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p]),
    "octic_seg_knn_bf16": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                   c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "octic_seg_knn_vote": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_int, c_i64, c_int, ctypes.POINTER(c_int), c_int, c_void_p,
                                   c_void_p]),
    "octic_knn_topk_plan": (c_int, [c_i64, c_i64, c_int, c_int, ctypes.POINTER(c_int)]),
    "octic_knn_topk_workspace_bytes": (c_i64, [c_i64, c_i64, c_int, c_int, c_int]),
    "octic_knn_topk": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_i64,
                               c_void_p, c_void_p]),
    "octic_knn_vote": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_int, c_void_p, c_i64, c_int, c_float, ctypes.POINTER(c_int),
                               c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "octic_topk_rank": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p,
                                c_void_p]),
    "octic_topk_count": (c_int, [c_void_p, c_i64, c_i64, c_int, c_i64, c_void_p, c_int, ctypes.POINTER(c_int), c_int, c_void_p,
                                 c_void_p]),
    "octic_mix_images": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "octic_mix_targets": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_void_p, c_void_p]),
    "octic_mix_bce": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                              c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "octic_mix_ce": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                             c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "octic_cosub_bce": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                                c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "octic_augment_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_augment_u8": (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_float] * 6 + [c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_dino_resize_coeffs": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_dino_resize_max_taps": (c_int, [c_int]),
    "octic_dino_resize_u8": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p]),
    "octic_dino_color_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "octic_dino_color_u8": (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_float] * 6 + [c_int, c_int, c_int, c_void_p, c_void_p]),
    "octic_crop_resize_max_taps": (c_int, [c_int]),
    "octic_crop_resize_rows": (c_int, []),
    "octic_crop_resize_u8": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_int] + [c_float] * 6 + [c_void_p]),
    "octic_depth_ok": (c_int, [c_int, c_int, c_int, c_int]),
    "octic_depth_plan": (c_int, [c_i64, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    # patch / patch_ldb / patch_ldr / cls / cls_ldb are HOST arrays of `layers` entries (PtrArray4 / I64Array4)
    "octic_depth_logits": (c_int, [c_void_p] * 5 + [c_int, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                    c_void_p]),
    "octic_depth_expect": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    "octic_max_filter_prep": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p]),
    "octic_max_filter_fwd": (c_int, [VP, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p]),
    "octic_max_filter_bwd_x": (c_int, [c_void_p, c_void_p, c_void_p, VP, c_i64, c_i64, c_int, c_int, c_void_p]),
    "octic_max_filter_bwd_ref_plan": (c_int, [c_i64, c_i64, c_int, ctypes.POINTER(c_int)]),
    "octic_max_filter_bwd_ref_workspace_bytes": (c_i64, [c_i64, c_i64, c_int]),
    "octic_max_filter_bwd_ref": (c_int, [c_void_p, c_void_p, VP, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_void_p]),
    "octic_canonize_fwd": (c_int, [VP, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p]),
    "octic_canonize_bwd": (c_int, [c_void_p, c_int, c_void_p, VP, c_i64, c_int, c_int, c_void_p]),
    "octic_poly_invariant_fwd": (c_int, [VP, c_void_p, c_i64, c_int, c_int, c_int, c_void_p]),
    "octic_poly_invariant_bwd": (c_int, [c_void_p, c_int, VP, VP, c_i64, c_int, c_int, c_void_p]),
}


def header_symbols():
    """Every function name declared in include/octic_hip.h."""
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(octic_[a-z0-9_]+)\s*\(", text)))


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"octic_vits_amd: HIP library {LIB_PATH} is missing. Build it with "
                "`python -m octic_vits_amd.build` (hipcc, --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported: fail loudly
            fn.restype, fn.argtypes = res, args
        if L.octic_abi_version() != ABI_VERSION:
            raise RuntimeError("octic_vits_amd: ABI version mismatch between _lib.py and liboctic_hip.so")
        _LIB = L
    return _LIB


def route_override(knob: int, value: int) -> int:
    """Force a kernel / tiling choice for an A/B or a test (0 = automatic); returns the previous value."""
    old = lib().octic_route_override(knob, value)
    if old < 0:
        raise ValueError(f"octic_route_override: unknown knob {knob}")
    _PLANS.clear()
    for drop in _ON_OVERRIDE:
        drop()
    return old


# What else was sized or chosen under the override table and so must not outlive it: callables run by every route_override
# (ops registers the drop of its split-K workspace cache - a workspace sized for a plan that splits nothing is 256 bytes, and a
# launch planned under a forced split would put tickets and slabs past its end).  Nothing here runs per launch.
_ON_OVERRIDE = []


def on_route_override(drop):
    """Run drop() after every route_override, with _PLANS already empty."""
    if drop not in _ON_OVERRIDE:
        _ON_OVERRIDE.append(drop)
    return drop


# The answers of the library's plan queries by (query, arguments): the eager step asks per call, and without this the attention
# query alone measured 1.3 - 1.9 ms per ViT-H step slower than before it existed (NOTES, 'Attention routing'; 3.6 us a query).
# An answer holds until the override table changes: route_override drops them all.
_PLANS = {}


def plan(query, *args):
    """The four ints an octic_*_plan query writes for these arguments, or None where it refuses them with OCTIC_ESHAPE."""
    key = (query, args)
    answer = _PLANS.get(key, 0)
    if answer == 0:
        out = (c_int * 4)()
        code = getattr(lib(), query)(*args, out)
        if code not in (0, -1):
            check(code)
        _PLANS[key] = answer = tuple(out) if code == 0 else None
    return answer


def attn_plan(T, hd, dtype=BF16, ld_in=0, ld_out=0, ld_grad=0):
    """octic_attn_plan: (forward kernel, its waves, what a phase-3 backward call runs, its waves) - ATTN_FWD_* / ATTN_BWD_*."""
    answer = plan("octic_attn_plan", dtype, T, hd, ld_in, ld_out, ld_grad)
    if answer is None:
        check(-1)
    return answer


def check(code: int):
    if code != 0:
        raise RuntimeError(f"octic HIP call failed ({code}): {lib().octic_strerror(code).decode()}")
