"""ctypes binding of libnesr_hip.so (the C ABI declared in include/nesr_hip.h).

There is deliberately no fallback: if the library is missing or a call fails, the caller gets
an exception (the reference turns exceptions from its ESRGAN backend into silent bicubic
results, nesr/nesr.py:815-843, so a quiet fallback here would be invisible).
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnesr_hip.so")

DTYPE_F32, DTYPE_BF16, DTYPE_F32_WINOGRAD, DTYPE_F32_SPLIT, DTYPE_F16 = 0, 1, 2, 3, 4
ROUND_TRUNC, ROUND_NEAREST = 0, 1
UPCONV_3X3, UPCONV_2X2 = 0, 1
CONV_KERNEL_NAMES = {0: None, 1: "generic", 2: "xl", 3: "winograd", 4: "f16-pair", 5: "upconv2x2"}   # NESR_CONV_KERNEL_*
CONV_LAST_GENERAL, CONV_LAST_NARROW = 0, 1
ACT_PRELU, ACT_RELU, ACT_LEAKYRELU = 0, 1, 2
LAB_FROM_LAB, LAB_LINEAR, LAB_FIRST_IS_BLUE, LAB_PLANAR = 1, 2, 4, 8
INTER_LINEAR, INTER_LANCZOS4 = 1, 4
INTER_NEAREST, INTER_CUBIC = 0, 2
ENSEMBLE_MAX = 8     # images per nesr_ensemble_u8
ALPHA_NETWORK, ALPHA_LINEAR = 0, 1
INPUT_12CH, INPUT_3CH_X4 = 0, 1
STAGE_RECT = 13      # ints per tile of nesr_stage_tile_plan
ORDER_RGB, ORDER_BGR = 0, 1

# name -> (restype, argtypes); must list every symbol include/nesr_hip.h declares
_c = ctypes
SIGNATURES = {
    "nesr_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_create_compact": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_finalize_weights": (_c.c_int, [_c.c_void_p]),
    "nesr_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_forward_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_forward_ragged": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "nesr_set_size_independent": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_reserve": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_preferred_batch": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_forward_flops": (_c.c_double, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_band_begin": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_band_rdb": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    "nesr_band_tail": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_band_rdb_phase": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_band_pack_edges": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_band_unpack_aprons": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_band_row_bytes": (_c.c_size_t, [_c.c_void_p]),
    "nesr_band_rows": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "nesr_band_link": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_band_unlink": (_c.c_int, [_c.c_void_p]),
    "nesr_band_link_state": (_c.c_int, [_c.c_void_p]),
    "nesr_band_set_staged": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_band_push_edges": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_band_land_aprons": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_band_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int]),
    "nesr_forward_banded_u8": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                          _c.POINTER(_c.c_void_p)]),
    "nesr_forward_banded": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(_c.c_void_p)]),
    "nesr_set_concurrent": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_set_fused": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_fused_state": (_c.c_int, [_c.c_void_p]),
    "nesr_rdb_chain_state": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_rdb_chain_table": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    "nesr_strip_schedule": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int), _c.c_int,
                                       _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    "nesr_set_upconv": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_upconv_state": (_c.c_int, [_c.c_void_p]),
    "nesr_set_conv_last": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_fold_upconv_weights": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_debug_fault": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_set_kernel_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_double)]),
    "nesr_check_status": (_c.c_int, [_c.c_void_p]),
    "nesr_check_range": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "nesr_destroy": (None, [_c.c_void_p]),
    "nesr_cut_tiles_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_paste_tiles_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int64), _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_void_p]),
    "nesr_comm_unique_id": (_c.c_int, [_c.c_void_p]),
    "nesr_comm_init": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_comm_destroy": (_c.c_int, [_c.c_void_p]),
    "nesr_forward_sharded_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_shard_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int),
                                   _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_nl_means_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_clahe_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_lab_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_gaussian_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_gaussian_taps": (_c.c_int, [_c.c_double, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_nl_means_weights": (_c.c_int, [_c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int),
                                         _c.POINTER(_c.c_int)]),
    "nesr_preprocess_scratch_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "nesr_preprocess_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_double, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_postprocess_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_resize_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int,
                                  _c.c_void_p]),
    "nesr_resize_u16": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int,
                                   _c.c_void_p]),
    "nesr_resize_f32": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int,
                                   _c.c_void_p]),
    "nesr_resize_taps": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_float), _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_resize_cv_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int,
                                     _c.c_void_p]),
    "nesr_resize_cv_taps": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_segment_enhance_scratch_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "nesr_segment_enhance_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                           _c.c_void_p]),
    "nesr_ensemble_u8": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_jpeg_scratch_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "nesr_jpeg_header": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_jpeg_encode_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                       _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_jpeg_scratch_bytes_ex": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_jpeg_header_ex": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_jpeg_encode_ex_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                          _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_jpeg_parse": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_jpeg_decode_scratch_bytes": (_c.c_size_t, [_c.c_void_p]),
    "nesr_jpeg_decode_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                       _c.c_void_p]),
    "nesr_jpeg_decode_last_launches": (_c.c_int, [_c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_png_bound": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_png_scratch_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_png_head": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_png_code_lengths": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_png_encode": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                   _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_png_parse": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "nesr_png_decode_scratch_bytes": (_c.c_size_t, [_c.c_void_p]),
    "nesr_png_decode": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_size_t,
                                   _c.c_void_p, _c.c_void_p]),
    "nesr_png_unfilter_scratch_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_png_unfilter": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_size_t,
                                     _c.c_void_p, _c.c_void_p]),
    "nesr_pack_frame": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p,
                                   _c.c_void_p]),
    "nesr_unpack_frame": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_int64,
                                     _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "nesr_frame_scratch_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_enhance_frame": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                      _c.c_void_p, _c.c_void_p]),
    "nesr_forward_nesr_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int64, _c.c_void_p]),
    "nesr_stage_route": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_stage_tile_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.POINTER(_c.c_int)]),
    "nesr_apply_esrgan_scratch_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "nesr_apply_esrgan_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_void_p, _c.c_size_t,
                                        _c.c_void_p, _c.c_void_p]),
    "nesr_conv3x3": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_conv3x3_up": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                   _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int]),
    "nesr_segformer_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                         _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.c_int, _c.c_int]),
    "nesr_segformer_destroy": (None, [_c.c_void_p]),
    "nesr_segformer_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_segformer_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_segformer_finalize": (_c.c_int, [_c.c_void_p]),
    "nesr_segformer_output_size": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_segformer_forward_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_segformer_segment_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                             _c.c_void_p]),
    "nesr_segformer_preprocess_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_segformer_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_segformer_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_pil_resize_u8": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "nesr_swin2sr_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int),
                                       _c.POINTER(_c.c_int), _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_double, _c.c_char_p,
                                       _c.c_char_p]),
    "nesr_swin2sr_destroy": (None, [_c.c_void_p]),
    "nesr_swin2sr_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_swin2sr_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_swin2sr_finalize": (_c.c_int, [_c.c_void_p]),
    "nesr_swin2sr_output_size": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_swin2sr_forward_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_swin2sr_upscale_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_swin2sr_tile_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                          _c.POINTER(_c.c_int), _c.POINTER(_c.c_int32), _c.c_size_t]),
    "nesr_swin2sr_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_swin2sr_upscale_tiled_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_swin2sr_overlap_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                             _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int32), _c.c_size_t]),
    "nesr_swin2sr_overlap_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_swin2sr_upscale_overlapped_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_swin2sr_forward_batch_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_swin2sr_set_timing":(_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_swin2sr_set_dtype": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_swin2sr_part_f32": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                         _c.c_void_p]),
    "nesr_swin2sr_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_vae_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_int, _c.c_int, _c.c_double,
                                   _c.c_char_p]),
    "nesr_vae_destroy": (None, [_c.c_void_p]),
    "nesr_vae_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_vae_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_vae_finalize": (_c.c_int, [_c.c_void_p]),
    "nesr_vae_output_size": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "nesr_vae_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_vae_decode_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_vae_decode_latents_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_vae_decode_latents_tiled_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                                    _c.c_void_p]),
    "nesr_vae_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_vae_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_unet_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_char_p),
                                    _c.POINTER(_c.c_char_p), _c.c_char_p, _c.POINTER(_c.c_int), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                    _c.c_int, _c.c_double, _c.c_int, _c.c_double, _c.c_int, _c.c_char_p]),
    "nesr_unet_destroy": (None, [_c.c_void_p]),
    "nesr_unet_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_unet_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_unet_finalize": (_c.c_int, [_c.c_void_p]),
    "nesr_unet_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_unet_forward_f32": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_void_p, _c.c_int,
                                         _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_unet_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_unet_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_unet_set_dtype": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_unet_dtype": (_c.c_int, [_c.c_void_p]),
    "nesr_unet_weight_bytes": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "nesr_unet_pack_linear_f16": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t]),
    "nesr_unet_pack_conv_f16": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t]),
    "nesr_unet_k_conv_f16": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.POINTER(_c.c_int), _c.c_void_p]),
    "nesr_unet_k_rows_f16": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.POINTER(_c.c_int), _c.c_void_p]),
    "nesr_unet_k_in": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_longlong, _c.c_void_p, _c.c_void_p]),
    "nesr_unet_k_embedding": (_c.c_int, [_c.c_double, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p]),
    "nesr_unet_k_temb": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_ulonglong), _c.POINTER(_c.c_ulonglong),
                                    _c.POINTER(_c.c_ulonglong), _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "nesr_unet_k_conv": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                    _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "nesr_unet_k_group_norm": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_void_p]),
    "nesr_unet_k_layer_norm_stats": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p]),
    "nesr_unet_k_rows": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                    _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p]),
    "nesr_unet_k_attention": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_void_p, _c.c_void_p]),
    "nesr_vae_k_in": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p]),
    "nesr_vae_k_conv": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                   _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "nesr_vae_k_group_norm": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_void_p,
                                         _c.c_void_p]),
    "nesr_vae_k_rows": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_vae_k_attention": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "nesr_clip_text_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                         _c.c_char_p]),
    "nesr_clip_text_destroy": (None, [_c.c_void_p]),
    "nesr_clip_text_num_tensors": (_c.c_int, [_c.c_void_p]),
    "nesr_clip_text_load_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "nesr_clip_text_finalize": (_c.c_int, [_c.c_void_p]),
    "nesr_clip_text_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_clip_text_encode_f32": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int32), _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "nesr_clip_text_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_clip_text_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_clip_text_k_embed": (_c.c_int, [_c.POINTER(_c.c_int32), _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_void_p]),
    "nesr_clip_text_k_attention": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_double, _c.c_char_p, _c.c_char_p,
                                    _c.c_int, _c.c_int, _c.c_int, _c.c_char_p, _c.c_double, _c.c_int, _c.c_char_p, _c.c_int]),
    "nesr_sdx4_destroy": (None, [_c.c_void_p]),
    "nesr_sdx4_workspace_bytes": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "nesr_sdx4_upscale_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int, _c.c_double, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_launches": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int64)]),
    "nesr_sdx4_tile_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                       _c.POINTER(_c.c_int), _c.POINTER(_c.c_int32), _c.c_size_t]),
    "nesr_sdx4_tiled_workspace_bytes": (_c.c_int, [_c.c_int] * 12 + [_c.POINTER(_c.c_size_t)]),
    "nesr_sdx4_upscale_tiled_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                              _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_set_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "nesr_sdx4_kernel_time_ms": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.c_int, _c.POINTER(_c.c_int64)]),
    "nesr_sdx4_schedule": (_c.c_int, [_c.c_int, _c.c_double, _c.c_double, _c.c_char_p, _c.c_char_p, _c.c_int, _c.c_int, _c.c_char_p, _c.c_int,
                                      _c.POINTER(_c.c_int), _c.POINTER(_c.c_double), _c.POINTER(_c.c_float)]),
    "nesr_sdx4_noise_coefficients": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_float)]),
    "nesr_sdx4_k_prepare": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_float, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_k_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.POINTER(_c.c_float), _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p]),
    "nesr_sdx4_k_window_gather": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_k_accumulate": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.c_float, _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_k_tiled_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_float), _c.c_void_p]),
    "nesr_sdx4_k_blend_add": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "nesr_sdx4_k_blend_finish": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "nesr_debug_last_conv_kernel": (_c.c_int, []),
    "nesr_last_error": (_c.c_char_p, []),
    "nesr_version": (_c.c_char_p, []),
}

_lib = None
_lock = threading.Lock()


ERR_ARG, ERR_RANGE, ERR_NOFIT, ERR_UNSUPPORTED, ERR_BADFILE = -1, -5, -6, -7, -8


class NesrHipError(RuntimeError):
    """A libnesr_hip.so call returned a negative status."""


class NesrRangeError(NesrHipError, FloatingPointError):
    """NESR_ERR_RANGE: the f16-pair fp32 form or the f16 form met a weight, input or activation that is non-finite or
    beyond +-65504 (the reference would carry it in float32; here it is an error, never a saturated image)."""


class NesrNoFitError(NesrHipError):
    """NESR_ERR_NOFIT: the JPEG or PNG file did not fit the output buffer; `needed` is the size the device reported."""

    def __init__(self, needed, cap, who="nesr_jpeg_encode_u8"):
        super().__init__(f"{who} failed ({ERR_NOFIT}): the file needs {needed} bytes, the buffer holds {cap}")
        self.needed = needed
        self.cap = cap


class NesrUnsupportedError(NesrHipError):
    """NESR_ERR_UNSUPPORTED: a valid JPEG file outside what the device decodes (progressive, arithmetic, 12 bits, 4 components, ...)."""


class NesrBadFileError(NesrHipError):
    """NESR_ERR_BADFILE: malformed marker segments, or a scan the device rejected (`status`: the bits of its status word)."""

    def __init__(self, msg, status=0):
        super().__init__(msg)
        self.status = status


JPEG_SAMPLING = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}       # NESR_JPEG_420 | 422 | 444


class JpegOpts(ctypes.Structure):
    """nesr_jpeg_opts"""
    _fields_ = [("quality", _c.c_int32), ("sampling", _c.c_int32), ("optimize", _c.c_int32), ("restart_interval", _c.c_int32)]


class JpegHuff(ctypes.Structure):
    """nesr_jpeg_huff"""
    _fields_ = [("look", _c.c_uint16 * 512), ("maxcode", _c.c_int32 * 18), ("valoff", _c.c_int32 * 17), ("vals", _c.c_uint8 * 256)]


class JpegInfo(ctypes.Structure):
    """nesr_jpeg_info"""
    _fields_ = [("H", _c.c_int32), ("W", _c.c_int32), ("C", _c.c_int32), ("hs", _c.c_int32), ("vs", _c.c_int32), ("restart_interval", _c.c_int32),
                ("mcus_x", _c.c_int32), ("mcus_y", _c.c_int32), ("scan_offset", _c.c_int64), ("scan_bytes", _c.c_int64), ("q", (_c.c_uint16 * 64) * 3),
                ("dc", JpegHuff * 3), ("ac", JpegHuff * 3)]


def jpeg_parse(data):
    """nesr_jpeg_parse on the file's bytes -> JpegInfo; NesrUnsupportedError / NesrBadFileError as the parser classifies the file."""
    data = bytes(data)
    info = JpegInfo()
    rc = load().nesr_jpeg_parse(data, len(data), ctypes.byref(info))
    if rc != 0:
        msg = load().nesr_last_error()
        text = f"nesr_jpeg_parse failed ({rc}): {msg.decode() if msg else '?'}"
        if rc == ERR_UNSUPPORTED:
            raise NesrUnsupportedError(text)
        if rc == ERR_BADFILE:
            raise NesrBadFileError(text)
        raise NesrHipError(text)
    return info


class PngSegment(ctypes.Structure):
    """nesr_png_segment"""
    _fields_ = [("offset", _c.c_int64), ("bytes", _c.c_int64), ("first", _c.c_int32), ("last", _c.c_int32)]


class PngInfo(ctypes.Structure):
    """nesr_png_info"""
    _fields_ = [("H", _c.c_int32), ("W", _c.c_int32), ("C", _c.c_int32), ("depth", _c.c_int32), ("contiguous", _c.c_int32), ("n_segments", _c.c_int32),
                ("stream_bytes", _c.c_int64), ("adler", _c.c_uint32)]


PNG_DEPENDENT = 16      # the status bit of nesr_png_decode that is no bad file: a distance that reaches before its segment


def png_parse(data, cap=None):
    """nesr_png_parse on the file's bytes -> (PngInfo, array of PngSegment); NesrUnsupportedError / NesrBadFileError as the parser
    classifies the file.  cap=None: the table is sized by a first call."""
    data = bytes(data)
    info = PngInfo()
    lib = load()
    segs = (PngSegment * max(cap, 1))() if cap is not None else None
    rc = lib.nesr_png_parse(data, len(data), ctypes.byref(info), segs, cap or 0)
    if rc == ERR_NOFIT and cap is None:
        segs = (PngSegment * info.n_segments)()
        rc = lib.nesr_png_parse(data, len(data), ctypes.byref(info), segs, info.n_segments)
    if rc != 0:
        msg = lib.nesr_last_error()
        text = f"nesr_png_parse failed ({rc}): {msg.decode() if msg else '?'}"
        if rc == ERR_UNSUPPORTED:
            raise NesrUnsupportedError(text)
        if rc == ERR_BADFILE:
            raise NesrBadFileError(text)
        err = NesrHipError(text)
        err.code, err.info = rc, info
        raise err
    return info, segs


def load():
    """Loads (once) and returns the ctypes handle; raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NesrHipError(
                f"{LIB_PATH} is missing: build it with `python -m neural_enhanced_super_resolution_amd.build` "
                "(hipcc, gfx950). There is no CPU or PyTorch fallback for this path.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)   # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().nesr_last_error()
        cls = NesrRangeError if rc == ERR_RANGE else NesrHipError
        raise cls(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
