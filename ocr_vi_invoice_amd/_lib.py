"""ctypes binding of libocrvi.so (include/ocrvi.h).  There is no CPU fallback: if the HIP library is
missing or fails to load, everything that needs it raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# (OCRVI_LIB: development aid -- an instrumented build of the same library, e.g. the ring-GEMM phase-stamp build tools/ring_prof.py uses)
LIB_PATH = os.environ.get("OCRVI_LIB") or os.path.join(_HERE, "lib", "libocrvi.so")

OCRVI_F32, OCRVI_BF16, OCRVI_F16, OCRVI_F16X2 = 0, 1, 2, 3
DTYPES = {"f32": OCRVI_F32, "fp32": OCRVI_F32, "float32": OCRVI_F32, "bf16": OCRVI_BF16, "bfloat16": OCRVI_BF16,
          "f16": OCRVI_F16, "fp16": OCRVI_F16, "float16": OCRVI_F16,
          # fp32-equivalent arithmetic on the 16-bit matrix pipe: every operand kept as two fp16 halves (include/ocrvi.h)
          "f16x2": OCRVI_F16X2}
ABI_VERSION = 5

EXPORTS = [
    "ocrvi_last_error", "ocrvi_abi_version",
    "ocrvi_det_create", "ocrvi_det_destroy", "ocrvi_det_workspace_bytes", "ocrvi_det_forward", "ocrvi_det_debug_features",
    "ocrvi_rec_create", "ocrvi_rec_destroy", "ocrvi_rec_workspace_bytes", "ocrvi_rec_forward", "ocrvi_rec_debug_features",
    "ocrvi_ctc_greedy", "ocrvi_normalize_u8", "ocrvi_resize_u8", "ocrvi_crop_resize_normalize", "ocrvi_db_postprocess", "ocrvi_db_boxes_batch",
    "ocrvi_unclip_polygon", "ocrvi_db_components_workspace_bytes", "ocrvi_db_components", "ocrvi_db_boxes_batch_sparse",
    "ocrvi_test_deform_conv", "ocrvi_test_offset_conv", "ocrvi_test_conv", "ocrvi_test_gemm", "ocrvi_test_attention", "ocrvi_test_mlp", "ocrvi_test_stem_pool", "ocrvi_test_pack_f16x2",
    "ocrvi_prof_enable", "ocrvi_prof_reset", "ocrvi_prof_report",
    "ocrvi_det_status", "ocrvi_rec_status", "ocrvi_range_reset", "ocrvi_range_flag",
    "ocrvi_resize_normalize_pages", "ocrvi_crop_resize_normalize_pages", "ocrvi_db_boxes_pages",
    "ocrvi_det_binary_workspace_bytes", "ocrvi_det_forward_binary",
    "ocrvi_four_point_transform", "ocrvi_warp_perspective_u8", "ocrvi_warp_perspective_pages",
    "ocrvi_test_layernorm", "ocrvi_test_frm_vertical", "ocrvi_test_asf", "ocrvi_test_maxpool", "ocrvi_test_db_maps", "ocrvi_test_ctc_logsoftmax",
    "ocrvi_det_eval_workspace_bytes", "ocrvi_det_eval", "ocrvi_ctc_loss", "ocrvi_edit_distance",
    "ocrvi_test_deform_conv_res",
    "ocrvi_enhance_init", "ocrvi_enhance_tables", "ocrvi_enhance_workspace_bytes", "ocrvi_enhance_u8",
    "ocrvi_rgb_to_lab_u8", "ocrvi_lab_to_rgb_u8", "ocrvi_clahe_lab_u8", "ocrvi_nlm_lab_u8", "ocrvi_sharpen_u8",
    "ocrvi_min_area_quads", "ocrvi_quad_crops", "ocrvi_crop_quad_resize_normalize_pages", "ocrvi_crop_quad_resize_normalize",
    "ocrvi_jpeg_info", "ocrvi_jpeg_parse", "ocrvi_jpeg_table_entry", "ocrvi_jpeg_decode_pages",
    "ocrvi_test_conv_res", "ocrvi_test_db_tail",
    "ocrvi_db_target_jobs", "ocrvi_db_target_maps", "ocrvi_resize_normalize_pad_pages",
    "ocrvi_test_mlp_raw", "ocrvi_test_lin_x2", "ocrvi_test_pack_stream", "ocrvi_test_swizzles", "ocrvi_test_persistent_grid",
    "ocrvi_test_bneck_tail",
    "ocrvi_jpeg_quant_tables", "ocrvi_jpeg_encode_header", "ocrvi_jpeg_encode_sizes", "ocrvi_jpeg_encode_table_entry", "ocrvi_jpeg_encode_pages",
    "ocrvi_test_gemm_raw", "ocrvi_test_ring_plan",
    "ocrvi_overlay_segments", "ocrvi_overlay_pages",
    "ocrvi_test_deform_conv_raw", "ocrvi_test_dcn_plan",
    "ocrvi_test_conv_raw", "ocrvi_test_gconv_plan",
    "ocrvi_png_info", "ocrvi_png_parse", "ocrvi_png_table_entry", "ocrvi_png_plan", "ocrvi_png_decode_pages",
    "ocrvi_png_encode_sizes", "ocrvi_png_encode_table_entry", "ocrvi_png_encode_pages", "ocrvi_test_png_code_lengths",
    "ocrvi_document_contour", "ocrvi_document_contour_bits", "ocrvi_doc_working_size", "ocrvi_doc_mask_sizes", "ocrvi_doc_mask_pages",
    "ocrvi_doc_grey_u8", "ocrvi_doc_smooth_u8", "ocrvi_doc_histogram", "ocrvi_doc_otsu", "ocrvi_doc_mask_bits",
    "ocrvi_rec_forward_conf", "ocrvi_ctc_greedy_conf", "ocrvi_test_ctc_logsoftmax_conf",
    "ocrvi_test_conv3_halo_raw", "ocrvi_test_bneck_tail_raw", "ocrvi_test_stem_pool_raw", "ocrvi_test_halo_plan",
    "ocrvi_ctc_beam_workspace_bytes", "ocrvi_ctc_beam",
    "ocrvi_lm_build", "ocrvi_lm_score", "ocrvi_lm_create", "ocrvi_lm_destroy", "ocrvi_ctc_beam_lm_workspace_bytes", "ocrvi_ctc_beam_lm",
    "ocrvi_skew_sizes", "ocrvi_skew_scores_pages", "ocrvi_skew_edges_u8", "ocrvi_skew_scores", "ocrvi_skew_pick", "ocrvi_skew_quad",
    "ocrvi_test_gconv_x2", "ocrvi_test_gconv_x2_plan",
]
PAGE_ENTRY = 4          # int64 fields of one page-table entry: (device address, height, width, 0) -- OCRVI_PAGE_ENTRY
# ocrvi_det_eval's record: 13 slots of 8 bytes (OCRVI_DET_EVAL_*), the first six int64, the rest float64
DET_EVAL_RECORD_BYTES = 104
DET_EVAL_INT_SLOTS = ("tp", "fp", "fn", "positive_count", "negatives", "negative_count")
DET_EVAL_F64_SLOTS = ("pos_bce", "topk_bce", "dice_inter", "pred_mask", "gt_mask", "l1_num", "thresh_mask")
CTC_LOSS_MAX_TARGET = 1024      # OCRVI_CTC_LOSS_MAX_TARGET
EDIT_DISTANCE_MAX_LEN = 2048    # OCRVI_EDIT_DISTANCE_MAX_LEN
CTC_BEAM_MAX = 64               # OCRVI_CTC_BEAM_MAX
CTC_BEAM_MAX_T = 1024           # OCRVI_CTC_BEAM_MAX_T
LM_MAX_ORDER = 6                # OCRVI_LM_MAX_ORDER
CLAHE_WORKSPACE_BYTES = 16384   # OCRVI_CLAHE_WORKSPACE_BYTES
ENHANCE_MIN_SIDE = 16           # the smallest page side the enhance entries take
DB_TARGET_GT, DB_TARGET_MASK, DB_TARGET_THRESH = 0, 1, 2   # OCRVI_DB_TARGET_*: the map a fill job writes
DB_TARGET_JOB = 8               # int32 fields of one fill job -- OCRVI_DB_TARGET_JOB
DB_TARGET_MAX_SIDE = 16384      # OCRVI_DB_TARGET_MAX_SIDE
JPEG_ENTRY = 64                 # int64 fields of one ocrvi_jpeg_decode_pages table entry -- OCRVI_JPEG_ENTRY
PNG_ENTRY = 16                  # int64 fields of one ocrvi_png_decode_pages table entry -- OCRVI_PNG_ENTRY
JPEG_ENC_ENTRY = 64             # int64 fields of one ocrvi_jpeg_encode_pages table entry -- OCRVI_JPEG_ENC_ENTRY
JPEG_HEADER_MAX = 640           # OCRVI_JPEG_HEADER_MAX
PNG_ENC_ENTRY = 16              # int64 fields of one ocrvi_png_encode_pages table entry -- OCRVI_PNG_ENC_ENTRY
PNG_ENC_BLOCK = 16384           # bytes of one deflate block -- OCRVI_PNG_ENC_BLOCK
OVERLAY_SEG = 8                 # int32 fields of one overlay segment -- OCRVI_OVERLAY_SEG
OVERLAY_PRIM = 8                # int32 fields of one overlay primitive -- OCRVI_OVERLAY_PRIM
OVERLAY_MAX_COORD = 16384       # OCRVI_OVERLAY_MAX_COORD: page sides 1..16384, endpoints within +-16384
DOC_POLARITIES = {"auto": 0, "bright": 1, "dark": 2}   # OCRVI_DOC_AUTO / _BRIGHT / _DARK
DOC_WORK_H = 500                # the reference's working height (scanner.py:85)
SKEW_K, SKEW_ANGLES = 128, 257  # OCRVI_SKEW_K, OCRVI_SKEW_ANGLES


class DetCfg(C.Structure):
    # backbone: 0 = ResNet-50, 1 = ResNet-18; no_dcn: 0 = DCN in layer2..4, 1 = plain 3x3 (a zeroed struct is ResNet-50 with DCN)
    _fields_ = [("dtype", C.c_int32), ("k", C.c_float), ("max_batch", C.c_int32), ("backbone", C.c_int32), ("no_dcn", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class RecCfg(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("dims", C.c_int32 * 3), ("num_blocks", C.c_int32 * 3), ("num_local", C.c_int32 * 3),
                ("num_classes", C.c_int32), ("blank_id", C.c_int32), ("reserved", C.c_int32 * 4)]


class JpegInfo(C.Structure):
    """ocrvi_jpeg_info_t"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32 * 3), ("v_samp", C.c_int32 * 3),
                ("restart_interval", C.c_int32), ("orientation", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32),
                ("reserved", C.c_int32), ("blocks", C.c_int64), ("stream_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("quant", (C.c_uint16 * 64) * 3), ("reason", C.c_char * 160)]


class PngInfo(C.Structure):
    """ocrvi_png_info_t"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("colour_type", C.c_int32), ("channels", C.c_int32),
                ("row_bytes", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32), ("palette_entries", C.c_int32),
                ("reserved", C.c_int32), ("idat_bytes", C.c_uint64), ("stream_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("reason", C.c_char * 160)]


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libocrvi.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ocr_vi_invoice_amd/csrc`).  There is no CPU fallback for the product path.")
    # torch must own the HIP runtime: importing it first makes libocrvi's libamdhip64 dependency resolve to the copy torch
    # already loaded, so streams, device pointers and the device context are shared (a second runtime sees no device).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i32, f32p, i32p, sz = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t
    lib.ocrvi_last_error.restype = C.c_char_p
    lib.ocrvi_last_error.argtypes = []
    lib.ocrvi_abi_version.restype = i32
    lib.ocrvi_det_create.argtypes = [i32, vp, sz, C.POINTER(DetCfg), C.POINTER(vp)]
    lib.ocrvi_det_destroy.argtypes = [vp]
    lib.ocrvi_det_destroy.restype = None
    lib.ocrvi_det_workspace_bytes.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_det_forward.argtypes = [vp, f32p, i32, i32, i32, f32p, f32p, f32p, f32p, f32p, vp, sz, vp]
    lib.ocrvi_det_binary_workspace_bytes.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_det_forward_binary.argtypes = [vp, f32p, i32, i32, i32, f32p, vp, sz, vp]
    lib.ocrvi_det_debug_features.argtypes = [vp, i32, i32, i32, f32p, f32p, f32p, f32p, f32p, vp, sz, vp]
    lib.ocrvi_rec_create.argtypes = [i32, vp, sz, C.POINTER(RecCfg), C.POINTER(vp)]
    lib.ocrvi_rec_destroy.argtypes = [vp]
    lib.ocrvi_rec_destroy.restype = None
    lib.ocrvi_rec_workspace_bytes.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_rec_forward.argtypes = [vp, f32p, i32, i32, i32, f32p, i32p, i32p, i32p, vp, sz, vp]
    lib.ocrvi_rec_debug_features.argtypes = [vp, i32, i32, i32, f32p, f32p, vp, sz, vp]
    lib.ocrvi_ctc_greedy.argtypes = [i32, f32p, i32, i32, i32, i32, i32p, i32p, i32p, vp]
    lib.ocrvi_rec_forward_conf.argtypes = [vp, f32p, i32, i32, i32, f32p, i32p, i32p, i32p, f32p, f32p, i32p, vp, sz, vp]
    lib.ocrvi_ctc_greedy_conf.argtypes = [i32, f32p, i32, i32, i32, i32, i32p, i32p, i32p, f32p, f32p, i32p, vp]
    lib.ocrvi_test_ctc_logsoftmax_conf.argtypes = [i32, f32p, i32, i32, i32, i32, f32p, i32p, f32p]
    lib.ocrvi_normalize_u8.argtypes = [i32, vp, i32, i32, i32, f32p, vp]
    lib.ocrvi_resize_u8.argtypes = [i32, vp, i32, i32, vp, i32, i32, vp]
    lib.ocrvi_crop_resize_normalize.argtypes = [i32, vp, i32, i32, i32, i32p, i32, i32, i32, f32p, vp]
    lib.ocrvi_db_postprocess.argtypes = [vp, i32, i32, C.c_float, C.c_float, i32, C.c_float, C.c_float, vp, i32, vp, vp, i32, C.POINTER(i32)]
    lib.ocrvi_db_components_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ocrvi_db_components_workspace_bytes.restype = sz
    lib.ocrvi_db_components.argtypes = [i32, vp, i32, i32, i32, C.c_float, vp, vp, vp, i32, vp, vp, C.c_longlong, vp, vp]
    lib.ocrvi_db_boxes_batch_sparse.argtypes = [vp, vp, vp, i32, vp, vp, C.c_longlong, i32, i32, i32, C.c_float, i32, C.c_float, C.c_float,
                                                C.c_double, C.c_double, i32, i32, i32, vp, vp, i32, vp, i32, vp]
    lib.ocrvi_unclip_polygon.argtypes = [vp, i32, C.c_double, vp, i32, C.POINTER(i32)]
    lib.ocrvi_db_boxes_batch.argtypes = [vp, i32, i32, i32, C.c_float, C.c_float, i32, C.c_float, C.c_float, C.c_double, C.c_double, i32, i32, i32,
                                         vp, vp, i32, vp, i32]
    lib.ocrvi_resize_normalize_pages.argtypes = [i32, vp, i32, i32, i32, f32p, vp]
    lib.ocrvi_crop_resize_normalize_pages.argtypes = [i32, vp, i32, i32p, i32, i32, i32, f32p, vp]
    lib.ocrvi_four_point_transform.argtypes = [vp, vp, vp, i32p, i32p]
    lib.ocrvi_warp_perspective_u8.argtypes = [i32, vp, i32, i32, vp, vp, i32, i32, vp]
    lib.ocrvi_warp_perspective_pages.argtypes = [i32, vp, vp, vp, i32, vp]
    lib.ocrvi_db_boxes_pages.argtypes = [vp, i32, i32, i32, C.c_float, C.c_float, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp,
                                         vp, i32, vp, vp, vp, i32, vp, vp, i32]
    lib.ocrvi_test_deform_conv.argtypes = [i32, i32, f32p, f32p, f32p, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32p, i32,
                                           C.POINTER(C.c_float)]
    lib.ocrvi_test_deform_conv_res.argtypes = [i32, i32, f32p, f32p, f32p, vp, vp, f32p, i32, i32, i32, i32, i32, i32, i32, f32p, i32,
                                               C.POINTER(C.c_float)]
    lib.ocrvi_test_offset_conv.argtypes = [i32, i32, f32p, vp, vp, i32, i32, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_conv.argtypes = [i32, i32, f32p, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32p, i32,
                                    C.POINTER(C.c_float)]
    lib.ocrvi_test_conv_res.argtypes = [i32, i32, f32p, vp, vp, f32p, i32, i32, i32, i32, i32, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_bneck_tail.argtypes = [i32, f32p, f32p, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32p, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_db_tail.argtypes = [i32, i32, f32p, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32p, f32p, i32,
                                       C.POINTER(C.c_float)]
    lib.ocrvi_test_gemm.argtypes = [i32, i32, f32p, vp, vp, f32p, i32, i32, i32, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_gemm_raw.argtypes = [i32, i32, f32p, vp, vp, f32p, i32, i32, i32, i32, i32, i32, vp, f32p]
    lib.ocrvi_test_ring_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32)]
    lib.ocrvi_test_deform_conv_raw.argtypes = [i32, i32, f32p, f32p, f32p, vp, vp, f32p, i32, i32, i32, i32, i32, i32, i32, vp, f32p]
    lib.ocrvi_test_dcn_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32)]
    lib.ocrvi_test_conv_raw.argtypes = [i32, i32, f32p, vp, vp, f32p] + [i32] * 13 + [vp, f32p]
    lib.ocrvi_test_gconv_plan.argtypes = [i32] * 12 + [C.POINTER(C.c_int32)]
    lib.ocrvi_test_gconv_x2.argtypes = [i32, f32p, vp, vp, f32p] + [i32] * 9 + [vp, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_gconv_x2_plan.argtypes = [i32] * 6 + [C.POINTER(C.c_int32)]
    lib.ocrvi_test_stem_pool.argtypes = [i32, i32, f32p, vp, vp, i32, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_conv3_halo_raw.argtypes = [i32, f32p, vp, vp, i32, i32, i32, i32, i32, i32, vp, f32p]
    lib.ocrvi_test_bneck_tail_raw.argtypes = [i32, f32p, f32p, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, f32p, f32p]
    lib.ocrvi_test_stem_pool_raw.argtypes = [i32, i32, f32p, vp, vp, i32, i32, i32, i32, vp, f32p]
    lib.ocrvi_test_halo_plan.argtypes = [i32] * 7 + [C.POINTER(C.c_int32)]
    lib.ocrvi_test_attention.argtypes = [i32, i32, f32p, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_mlp.argtypes = [i32, i32, f32p, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_lin_x2.argtypes = [i32, f32p, vp, vp, i32, i32, i32, i32, vp, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_mlp_raw.argtypes = [i32, i32, f32p, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, f32p, i32, C.POINTER(C.c_float)]
    lib.ocrvi_test_pack_f16x2.argtypes = [f32p, sz, vp, C.POINTER(C.c_float)]
    lib.ocrvi_test_pack_stream.argtypes = [i32, vp, vp, i32, i32, vp, sz, C.POINTER(sz), C.POINTER(C.c_float)]
    lib.ocrvi_test_swizzles.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ocrvi_test_persistent_grid.argtypes = [i32, i32, C.POINTER(C.c_int32)]
    lib.ocrvi_test_layernorm.argtypes = [i32, i32, f32p, i32, i32, vp, vp, i32, i32, f32p]
    lib.ocrvi_test_frm_vertical.argtypes = [i32, i32, f32p, vp, i32, i32, i32, i32, f32p]
    lib.ocrvi_test_asf.argtypes = [i32, i32, f32p, f32p, f32p, f32p, vp, vp, i32, i32, i32, f32p]
    lib.ocrvi_test_maxpool.argtypes = [i32, i32, f32p, i32, i32, i32, i32, f32p]
    lib.ocrvi_test_db_maps.argtypes = [i32, f32p, f32p, C.c_float, f32p, f32p, f32p, sz]
    lib.ocrvi_test_ctc_logsoftmax.argtypes = [i32, f32p, i32, i32, i32, i32, f32p, i32p]
    lib.ocrvi_det_eval_workspace_bytes.argtypes = [i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_det_eval.argtypes = [i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, i32, C.c_double, vp, vp, sz, vp]
    lib.ocrvi_ctc_loss.argtypes = [i32, f32p, i32, i32, i32, i32p, i32, i32p, i32p, i32, vp, vp]
    lib.ocrvi_edit_distance.argtypes = [i32, i32p, i32, i32p, i32p, i32, i32p, i32, i32p, vp]
    lib.ocrvi_ctc_beam_workspace_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_ctc_beam.argtypes = [i32, f32p, i32, i32, i32, i32, i32, i32, i32p, i32p, vp, vp, sz, vp]
    lib.ocrvi_lm_build.argtypes = [i32p, i32p, f32p, f32p, sz, i32, i32, i32, C.c_double, vp, sz, C.POINTER(sz)]
    lib.ocrvi_lm_score.argtypes = [vp, sz, i32p, i32, C.POINTER(C.c_double), vp]
    lib.ocrvi_lm_create.argtypes = [i32, vp, sz, C.POINTER(vp)]
    lib.ocrvi_lm_destroy.argtypes = [vp]
    lib.ocrvi_lm_destroy.restype = None
    lib.ocrvi_ctc_beam_lm_workspace_bytes.argtypes = [i32, i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_ctc_beam_lm.argtypes = [i32, f32p, i32, i32, i32, i32, i32, i32, vp, C.c_double, C.c_double, i32p, i32p, vp, vp, vp, vp, sz, vp]
    lib.ocrvi_enhance_init.argtypes = [i32]
    lib.ocrvi_enhance_tables.argtypes = [vp, sz, C.POINTER(sz)]
    lib.ocrvi_enhance_workspace_bytes.argtypes = [i32, i32, C.POINTER(sz)]
    lib.ocrvi_enhance_u8.argtypes = [i32, vp, i32, i32, vp, vp, sz, vp]
    for name in ("ocrvi_rgb_to_lab_u8", "ocrvi_lab_to_rgb_u8", "ocrvi_nlm_lab_u8", "ocrvi_sharpen_u8"):
        getattr(lib, name).argtypes = [i32, vp, i32, i32, vp, vp]
    lib.ocrvi_clahe_lab_u8.argtypes = [i32, vp, i32, i32, vp, vp, sz, vp]
    lib.ocrvi_min_area_quads.argtypes = [vp, vp, i32, vp, vp]
    lib.ocrvi_quad_crops.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.ocrvi_crop_quad_resize_normalize_pages.argtypes = [i32, vp, i32, i32p, vp, i32, i32, i32, f32p, vp]
    lib.ocrvi_crop_quad_resize_normalize.argtypes = [i32, vp, i32, i32, i32, i32p, vp, i32, i32, i32, f32p, vp]
    lib.ocrvi_jpeg_info.argtypes = [vp, sz, C.POINTER(JpegInfo)]
    lib.ocrvi_jpeg_parse.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    lib.ocrvi_jpeg_table_entry.argtypes = [C.POINTER(JpegInfo), sz, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ocrvi_jpeg_decode_pages.argtypes = [i32, vp, vp, i32, vp, vp, sz, vp]
    lib.ocrvi_png_info.argtypes = [vp, sz, C.POINTER(PngInfo)]
    lib.ocrvi_png_parse.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    lib.ocrvi_png_table_entry.argtypes = [C.POINTER(PngInfo), sz, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ocrvi_png_plan.argtypes = [C.POINTER(PngInfo), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.ocrvi_png_decode_pages.argtypes = [i32, vp, vp, i32, vp, vp, sz, vp]
    lib.ocrvi_jpeg_quant_tables.argtypes = [i32, vp, vp]
    lib.ocrvi_jpeg_encode_header.argtypes = [i32, i32, i32, i32, i32, vp, sz, C.POINTER(sz)]
    lib.ocrvi_jpeg_encode_sizes.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.ocrvi_jpeg_encode_table_entry.argtypes = [i32, i32, i32, i32, i32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ocrvi_jpeg_encode_pages.argtypes = [i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.ocrvi_png_encode_sizes.argtypes = [i32, i32, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.ocrvi_png_encode_table_entry.argtypes = [i32, i32, i32, i32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ocrvi_png_encode_pages.argtypes = [i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.ocrvi_test_png_code_lengths.argtypes = [i32, vp, i32, i32, i32, vp, vp]
    lib.ocrvi_document_contour.argtypes = [vp, i32, i32, C.c_int64, vp, C.POINTER(C.c_int32)]
    lib.ocrvi_document_contour_bits.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_int32)]
    lib.ocrvi_doc_working_size.argtypes = [i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.ocrvi_doc_mask_sizes.argtypes = [i32, i32, i32, C.POINTER(sz), C.POINTER(sz)]
    lib.ocrvi_doc_mask_pages.argtypes = [i32, vp, i32, i32, i32, i32, vp, vp, sz, vp]
    lib.ocrvi_doc_grey_u8.argtypes = [i32, vp, i32, i32, i32, vp, vp]
    lib.ocrvi_doc_smooth_u8.argtypes = [i32, vp, i32, i32, vp, vp]
    lib.ocrvi_doc_histogram.argtypes = [i32, vp, i32, i32, vp, vp]
    lib.ocrvi_doc_otsu.argtypes = [i32, vp, vp, i32, i32, i32, vp, vp]
    lib.ocrvi_doc_mask_bits.argtypes = [i32, vp, i32, i32, vp, vp, vp]
    lib.ocrvi_skew_sizes.argtypes = [i32, i32, i32, C.POINTER(sz)]
    lib.ocrvi_skew_scores_pages.argtypes = [i32, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.ocrvi_skew_edges_u8.argtypes = [i32, vp, i32, i32, vp, vp]
    lib.ocrvi_skew_scores.argtypes = [i32, vp, i32, i32, vp, vp]
    lib.ocrvi_skew_pick.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ocrvi_skew_quad.argtypes = [i32, i32, i32, vp]
    lib.ocrvi_overlay_segments.argtypes = [vp, vp, vp, vp, vp, i32, C.c_uint32, C.c_uint32, i32, vp, C.c_int64, vp, C.c_int64, vp,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.ocrvi_overlay_pages.argtypes = [i32, vp, i32, vp, vp, vp, i32, i32, vp]
    lib.ocrvi_db_target_jobs.argtypes = [vp, vp, vp, vp, i32, C.c_double, i32, vp, i32, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), i32]
    lib.ocrvi_db_target_maps.argtypes = [i32, vp, i32, vp, i32, vp, i32, i32, C.c_float, f32p, f32p, f32p, f32p, vp]
    lib.ocrvi_resize_normalize_pad_pages.argtypes = [i32, vp, vp, i32, i32, f32p, vp]
    lib.ocrvi_det_status.argtypes = [vp]
    lib.ocrvi_rec_status.argtypes = [vp]
    lib.ocrvi_range_reset.argtypes = [i32, vp]
    lib.ocrvi_range_flag.argtypes = [i32, C.POINTER(i32)]
    lib.ocrvi_prof_enable.argtypes = [i32]
    lib.ocrvi_prof_reset.argtypes = []
    lib.ocrvi_prof_report.argtypes = [C.c_char_p, sz]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("ocrvi_last_error", "ocrvi_det_destroy", "ocrvi_rec_destroy", "ocrvi_lm_destroy"):
            fn.restype = i32
    if lib.ocrvi_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libocrvi ABI {lib.ocrvi_abi_version()} != binding {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def last_error() -> str:
    return load().ocrvi_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    """0 ok; OCRVI_EINVAL -> ValueError (shape/argument), OCRVI_ENOMEM -> MemoryError, OCRVI_ERANGE -> OverflowError (an f16x2 activation
    left fp16's exponent range), anything else -> RuntimeError."""
    if rc == 0:
        return
    msg = last_error()
    if rc == -1:
        raise ValueError(msg)
    if rc == -3:
        raise MemoryError(msg)
    if rc == -5:
        raise OverflowError(msg)
    raise RuntimeError(f"libocrvi error {rc}: {msg}")


def dtype_code(dtype) -> int:
    if isinstance(dtype, int):
        return dtype
    try:
        return DTYPES[str(dtype).replace("torch.", "")]
    except KeyError:
        raise ValueError(f"unsupported compute dtype {dtype!r}; choose from f32, f16x2, bf16, f16") from None


def ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def prof_report() -> dict:
    """Aggregated per-kernel-tag timings recorded since the last reset (see ocrvi_prof_report)."""
    import json
    buf = C.create_string_buffer(1 << 20)
    check(load().ocrvi_prof_report(buf, len(buf)))
    return json.loads(buf.value.decode())
