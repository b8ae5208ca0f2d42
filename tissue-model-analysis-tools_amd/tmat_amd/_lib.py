"""ctypes binding of libtmat_hip.so (include/tmat.h).

The HIP library is the product path.  There is no CPU fallback: if the shared object is missing
or no MI355X is visible, loading / `create()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("TMAT_HIP_LIB", _HERE / "libtmat_hip.so"))

_lib = None


class TmatError(RuntimeError):
    pass


E_ARG = -1          # TMAT_E_ARG (include/tmat.h): bad argument / unsupported shape
E_CAP = -4          # TMAT_E_CAP (include/tmat.h): a caller-provided output capacity is too small


class Row(C.Structure):
    _fields_ = [("index", C.c_int64), ("count", C.c_int64), ("total_px", C.c_double), ("avg_px", C.c_double)]


class AnalyzeOpts(C.Structure):
    """tmat_analyze_opts (include/tmat.h)"""
    _fields_ = [("size", C.c_uint32), ("ds_ratio", C.c_double), ("ds_width", C.c_int), ("graph_thresh_1", C.c_float), ("graph_thresh_2", C.c_float),
                ("smoothing_window_px", C.c_int), ("min_branch_length_px", C.c_int), ("max_branch_length_px", C.c_int), ("remove_isolated", C.c_int),
                ("first_index", C.c_int64), ("well_masks", C.c_void_p), ("pruning_masks", C.c_void_p), ("vis_width", C.c_int),
                ("rgb_out", C.c_void_p), ("bars_out", C.c_void_p), ("cap_b", C.c_int), ("n_bars", C.c_void_p), ("stage_out", C.c_void_p)]


class GridOpts(C.Structure):
    """tmat_grid_opts (include/tmat.h)"""
    _fields_ = [("size", C.c_uint32), ("n_thresh", C.c_int), ("thresh", C.c_void_p), ("tree_png", C.c_void_p), ("tree_png_cap", C.c_size_t),
                ("tree_png_sizes", C.c_void_p), ("barcode_png", C.c_void_p), ("barcode_png_cap", C.c_size_t), ("barcode_png_sizes", C.c_void_p)]


class StackOpts(C.Structure):
    """tmat_stack_opts (include/tmat.h)"""
    _fields_ = [("size", C.c_uint32), ("ds_width", C.c_int), ("hessian", C.c_int), ("n_thresh", C.c_int), ("thresh", C.c_void_p),
                ("smoothing_window_px", C.c_int), ("min_branch_length_px", C.c_int), ("max_branch_length_px", C.c_int), ("remove_isolated", C.c_int),
                ("first_index", C.c_int64), ("pruning_masks", C.c_void_p), ("fields_out", C.c_void_p), ("proj_pic_out", C.c_void_p),
                ("field_pic_out", C.c_void_p), ("pass_stacks", C.c_int),
                ("vis_width", C.c_int), ("rgb_out", C.c_void_p), ("bars_out", C.c_void_p), ("cap_b", C.c_int), ("n_bars", C.c_void_p)]


STACK_OPTS_SIZE_V1 = 88              # TMAT_STACK_OPTS_SIZE_V1: the struct before the tree request, still accepted


STACK_PASS_MAX = 8                   # TMAT_STACK_PASS_MAX
STACK_PASS_BUDGET = 8 << 30          # TMAT_STACK_PASS_BUDGET: device bytes of one pass of tmat_analyze_stack_batch
PIC_DTYPES = {np.dtype(np.uint16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.uint8): 3}      # TMAT_PIC_*
STAGE_PLANES = ("original", "prediction", "mask", "weighted")                                                       # TMAT_STAGE_*


def lib():
    """Load libtmat_hip.so once; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise TmatError(
            f"{LIB_PATH} not found: build it with `python tools/build.py` "
            "(hipcc --offload-arch=gfx950). tmat_amd has no CPU fallback.")
    L = C.CDLL(str(LIB_PATH))
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.tmat_last_error.restype = C.c_char_p
    L.tmat_version.restype = i
    L.tmat_create.argtypes = [i, vp, sz, i, C.POINTER(vp)]
    L.tmat_create_plain.argtypes = [i, C.POINTER(vp)]
    L.tmat_destroy.argtypes = [vp]
    L.tmat_destroy.restype = None
    L.tmat_sync.argtypes = [vp]
    L.tmat_set_input_depth.argtypes = [vp, i]
    L.tmat_unet_predict.argtypes = [vp, vp, i, vp]
    L.tmat_predict_smooth.argtypes = [vp, vp, i, i, i, vp]
    L.tmat_predict_smooth_ex.argtypes = [vp, vp, i, i, i, i, vp]
    L.tmat_smooth_plan.argtypes = [i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.tmat_spline_window.argtypes = [i, vp]
    L.tmat_smooth_begin.argtypes = [vp, vp, i, i, i, i, C.POINTER(i)]
    L.tmat_smooth_tiles.argtypes = [vp, i, i, vp]
    L.tmat_smooth_put.argtypes = [vp, i, i, vp, i]
    L.tmat_smooth_end.argtypes = [vp, vp]
    L.tmat_debug_smooth_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tmat_resize_pil_f32.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.tmat_host_resize_pil_f32.argtypes = [vp, i, i, i, i, i, i, vp]
    L.tmat_predict_auto_resample.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.tmat_segment_batch.argtypes = [vp, vp, i, i, i, C.c_double, vp]
    L.tmat_postprocess_batch.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_filter_edt_batch.argtypes = [vp, vp, i, i, i, vp, vp]
    L.tmat_medial_axis_batch.argtypes = [vp, vp, i, i, i, vp, vp]
    L.tmat_finish_batch.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp]
    L.tmat_filter_mask_batch.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_debug_filter_stages.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.tmat_debug_medial_stages.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, vp]
    L.tmat_gather_rows.argtypes = [vp, vp, i, vp, vp]
    L.tmat_zproj_batch.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_zproj_dev.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_dmt_graph.argtypes = [vp, vp, i, i, f, f, vp, i, vp, i, C.POINTER(i), C.POINTER(i)]
    L.tmat_dmt_graph_batch.argtypes = [vp, vp, i, i, i, f, f, vp, i, vp, i, vp, vp]
    L.tmat_morse_stats.argtypes = [vp, i, vp, i, i, i, i, i, i, i, vp, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), vp, i]
    L.tmat_morse_tree.argtypes = [vp, i, vp, i, i, i, i, i, i, i, vp, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), vp, vp, i, vp, i, C.POINTER(i), C.POINTER(i)]
    L.tmat_branch_color.argtypes = [i, vp]
    L.tmat_render_tree.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, i, vp]
    L.tmat_render_tree_timed.argtypes = L.tmat_render_tree.argtypes + [vp]
    L.tmat_host_render_tree.argtypes = [vp, i, i, i, i, vp, vp, vp, i, vp]
    L.tmat_host_render_barcode.argtypes = [vp, i, i, vp]
    L.tmat_analyze_batch_dev.argtypes = [vp, vp, i, i, i, C.c_double, i, f, f, i, i, i, i, C.c_int64, vp]
    L.tmat_analyze_batch.argtypes = [vp, vp, i, i, i, C.c_double, i, f, f, i, i, i, i, C.c_int64, vp]
    L.tmat_analyze_batch_tree_dev.argtypes = L.tmat_analyze_batch_dev.argtypes + [i, vp, vp, i, vp]
    L.tmat_analyze_batch_tree.argtypes = L.tmat_analyze_batch.argtypes + [i, vp, vp, i, vp]
    L.tmat_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.tmat_dev_free.argtypes = [vp, vp]
    L.tmat_dev_upload.argtypes = [vp, vp, vp, sz]
    L.tmat_dev_download.argtypes = [vp, vp, vp, sz]
    d = C.c_double
    L.tmat_set_gaussian_table.argtypes = [vp, d, i, i, vp]
    L.tmat_host_gaussian_kernel1d.argtypes = [d, i, i, vp]
    L.tmat_gaussian_f32.argtypes = [vp, vp, i, i, i, d, i, vp]
    L.tmat_sato_batch.argtypes = [vp, vp, i, i, i, vp, i, i, vp]
    L.tmat_stack_prepare.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_vessel_field.argtypes = [vp, vp, i, i, i, i, vp, vp]
    L.tmat_analyze_stack.argtypes = [vp, vp, i, i, i, i, i, f, f, i, i, i, i, C.c_int64, vp, vp]
    L.tmat_field_stats.argtypes = [vp, vp, i, i, f, f, i, i, i, i, C.c_int64, vp]
    L.tmat_field_stats_pruned.argtypes = [vp, vp, i, i, f, f, i, i, i, i, vp, C.c_int64, vp]
    L.tmat_resize_aa_u16.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_analyze_stack_batch.argtypes = [vp, vp, i, i, i, i, C.POINTER(StackOpts), vp]
    L.tmat_analyze_stack_batch_dev.argtypes = L.tmat_analyze_stack_batch.argtypes
    L.tmat_vessel_field_batch.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    L.tmat_stack_pass_plan.argtypes = [i, i, i, i, i, i, C.POINTER(i), C.POINTER(C.c_uint64)]
    L.tmat_debug_stack_trace.argtypes = [vp, i, C.POINTER(i), vp, vp]
    L.tmat_cell_area_batch.argtypes = [vp, vp, i, i, i, i, i, d, vp, vp, vp]
    L.tmat_cell_area_masked.argtypes = [vp, vp, vp, i, i, i, d, vp, vp, vp]
    L.tmat_resize_linear_u16.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_cell_small_dev.argtypes = [vp, vp, i, i, i, i, i, i, i, vp]
    L.tmat_cell_well_front_dev.argtypes = [vp, vp, i, i, i, i, vp, vp]
    L.tmat_cell_area_fit_dev.argtypes = [vp, vp, vp, i, i, i, d, vp, vp, vp]
    L.tmat_resnet_load.argtypes = [vp, vp, sz, C.POINTER(i)]
    L.tmat_resnet_predict.argtypes = [vp, i, vp, i, i, vp]
    L.tmat_inv_depth_predict.argtypes = [vp, vp, i, vp, i, i, i, i, vp, vp]
    L.tmat_inv_depth_predict_multi.argtypes = [vp, vp, i, vp, vp, i, i, i, i, vp]
    L.tmat_resnet_set_precision.argtypes = [vp, i]
    L.tmat_conv2d.argtypes = [vp, i, vp, i, i, i, i, vp, i, i, i, vp, vp, vp, i, i, vp]
    L.tmat_conv2d_roi.argtypes = [vp, vp, i, i, i, i, vp, i, i, i, vp, vp, vp, i, i, i, vp, i, vp, vp]
    L.tmat_conv2d_narrow.argtypes = [vp, vp, i, i, i, i, vp, i, i, i, i, vp, vp, vp, i, i, i, vp, i, vp, vp]
    L.tmat_model_layers.argtypes = [vp, sz, i, vp, C.POINTER(i)]
    L.tmat_prof_enable.argtypes = [vp, i]
    L.tmat_debug_poison.argtypes = [vp, i]
    L.tmat_debug_held_bytes.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.tmat_set_precision.argtypes = [vp, i]
    L.tmat_set_input_norm.argtypes = [vp, i, C.c_double, C.c_double]
    L.tmat_preprocess_batch.argtypes = [vp, vp, i, i, i, C.c_double, vp]
    L.tmat_well_threshold.argtypes = [vp, vp, i, i, vp]
    L.tmat_well_threshold_f64.argtypes = [vp, vp, i, i, vp]
    L.tmat_canny_mask.argtypes = [vp, vp, i, i, C.c_double, vp]
    L.tmat_canny_mask_batch.argtypes = [vp, vp, i, i, i, C.c_double, vp]
    L.tmat_well_small_shape.argtypes = [i, i, C.POINTER(i), C.POINTER(i)]
    L.tmat_stack_well_front_dev.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, vp]
    L.tmat_superellipse_table.argtypes = [vp, vp, i]
    L.tmat_superellipse_search.argtypes = [vp, vp, vp, i, vp, vp, vp, i, C.POINTER(i)]
    L.tmat_superellipse_masks.argtypes = [vp, vp, i, vp, vp, vp, i, i, vp, vp, i, C.POINTER(i)]
    L.tmat_resize_nearest_u8.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.tmat_analyze_batch_masked.argtypes = [vp, vp, i, i, i, C.c_double, i, f, f, i, i, i, i, C.c_int64, vp, vp, vp]
    L.tmat_analyze_batch_ex.argtypes = [vp, vp, i, i, i, C.POINTER(AnalyzeOpts), vp]
    L.tmat_analyze_batch_ex_dev.argtypes = [vp, vp, i, i, i, C.POINTER(AnalyzeOpts), vp]
    L.tmat_analyze_batch_grid.argtypes = [vp, vp, i, i, i, C.POINTER(AnalyzeOpts), C.POINTER(GridOpts), vp]
    L.tmat_analyze_batch_grid_dev.argtypes = [vp, vp, i, i, i, C.POINTER(AnalyzeOpts), C.POINTER(GridOpts), vp]
    L.tmat_render_barcode.argtypes = [vp, vp, vp, i, i, vp]
    L.tmat_render_barcode_png.argtypes = [vp, vp, vp, i, i, vp, sz, vp]
    L.tmat_host_barcode_rects.argtypes = [vp, i, i, vp, i, C.POINTER(i)]
    L.tmat_stage_pictures.argtypes = [vp, vp, i, i, sz, vp]
    L.tmat_host_stage_pictures.argtypes = [vp, i, i, sz, vp]
    L.tmat_png_stripe.argtypes = []
    L.tmat_png_bound.argtypes = [i, i, i, C.POINTER(sz)]
    L.tmat_png_encode_batch.argtypes = [vp, vp, i, i, i, i, vp, sz, vp]
    L.tmat_png_encode_batch_dev.argtypes = L.tmat_png_encode_batch.argtypes
    L.tmat_png_encode_batch_timed.argtypes = L.tmat_png_encode_batch.argtypes + [vp]
    L.tmat_host_png_encode_batch.argtypes = [vp, i, i, i, i, vp, sz, vp]
    L.tmat_host_png_encode_batch_mode.argtypes = [vp, i, i, i, i, vp, sz, vp, i]
    L.tmat_png_set_mode.argtypes = [vp, i]
    L.tmat_host_png_code_lengths.argtypes = [vp, i, i, vp]
    L.tmat_debug_png_code_lengths.argtypes = [vp, vp, i, i, i, vp]
    L.tmat_render_tree_png.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, i, vp, sz, vp]
    L.tmat_tiff_probe.argtypes = [vp, sz, i, vp, C.POINTER(i)]
    L.tmat_host_tiff_decode_batch.argtypes = [vp, vp, vp, vp, i, i, i, vp, C.POINTER(i), vp]
    L.tmat_tiff_decode_batch.argtypes = [vp] + L.tmat_host_tiff_decode_batch.argtypes
    L.tmat_tiff_decode_batch_dev.argtypes = L.tmat_tiff_decode_batch.argtypes
    L.tmat_tiff_decode_batch_dev_timed.argtypes = L.tmat_tiff_decode_batch.argtypes + [vp]
    L.tmat_prof_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), i]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("tmat_last_error", "tmat_destroy"):
            fn.restype = i
    _lib = L
    return L


EXPORTS = [
    "tmat_last_error", "tmat_version", "tmat_create", "tmat_create_plain", "tmat_destroy", "tmat_sync", "tmat_set_input_depth", "tmat_unet_predict",
    "tmat_predict_smooth", "tmat_segment_batch", "tmat_postprocess_batch", "tmat_filter_edt_batch", "tmat_medial_axis_batch", "tmat_finish_batch", "tmat_filter_mask_batch", "tmat_zproj_batch", "tmat_zproj_dev", "tmat_gather_rows",
    "tmat_dmt_graph", "tmat_dmt_graph_batch", "tmat_morse_stats",
    "tmat_morse_tree", "tmat_branch_color", "tmat_render_tree", "tmat_render_tree_timed", "tmat_host_render_tree", "tmat_host_render_barcode",
    "tmat_analyze_batch_dev", "tmat_analyze_batch", "tmat_analyze_batch_tree_dev", "tmat_analyze_batch_tree", "tmat_dev_alloc", "tmat_dev_free", "tmat_dev_upload", "tmat_dev_download",
    "tmat_prof_enable", "tmat_prof_read", "tmat_debug_poison", "tmat_debug_held_bytes", "tmat_debug_filter_stages", "tmat_debug_medial_stages", "tmat_set_precision", "tmat_set_input_norm", "tmat_preprocess_batch", "tmat_well_threshold", "tmat_well_threshold_f64", "tmat_canny_mask", "tmat_superellipse_table", "tmat_superellipse_search",
    "tmat_superellipse_masks", "tmat_resize_nearest_u8", "tmat_analyze_batch_masked", "tmat_host_lanczos4_u16", "tmat_host_rescale01_u16",
    "tmat_host_rescale255_f32", "tmat_host_filter_mask", "tmat_host_skeletonize", "tmat_host_medial_axis",
    "tmat_host_permutation", "tmat_host_postprocess",
    "tmat_set_gaussian_table", "tmat_host_gaussian_kernel1d", "tmat_gaussian_f32", "tmat_sato_batch", "tmat_stack_prepare", "tmat_vessel_field",
    "tmat_analyze_stack", "tmat_field_stats", "tmat_field_stats_pruned", "tmat_resize_aa_u16", "tmat_cell_area_batch", "tmat_cell_area_masked", "tmat_resize_linear_u16",
    "tmat_resnet_load", "tmat_resnet_predict", "tmat_inv_depth_predict", "tmat_inv_depth_predict_multi", "tmat_resnet_set_precision", "tmat_conv2d",
    "tmat_roi_plan", "tmat_roi_plan_tight", "tmat_roi_plan_exact", "tmat_conv2d_roi", "tmat_conv2d_roi_s2", "tmat_roi_plan_down", "tmat_roi_sep_tiles", "tmat_debug_sep_tiles", "tmat_debug_down_segs", "tmat_debug_down_seg_total",
    "tmat_roi_plan_const", "tmat_roi_sep_tiles_live", "tmat_roi_plan_share", "tmat_roi_sep_tiles_share", "tmat_roi_plan_share_rect", "tmat_roi_plan_share_fused_rect", "tmat_roi_down_schedule", "tmat_debug_share_fill_check",
    "tmat_stage_pictures", "tmat_host_stage_pictures", "tmat_analyze_batch_ex", "tmat_analyze_batch_ex_dev",
    "tmat_png_stripe", "tmat_png_bound", "tmat_png_encode_batch", "tmat_png_encode_batch_dev", "tmat_png_encode_batch_timed",
    "tmat_host_png_encode_batch", "tmat_render_tree_png",
    "tmat_analyze_stack_batch", "tmat_vessel_field_batch", "tmat_stack_pass_plan", "tmat_debug_stack_trace",
    "tmat_analyze_batch_grid", "tmat_analyze_batch_grid_dev", "tmat_render_barcode", "tmat_render_barcode_png", "tmat_host_barcode_rects",
    "tmat_analyze_stack_batch_dev", "tmat_canny_mask_batch", "tmat_well_small_shape", "tmat_stack_well_front_dev",
    "tmat_cell_small_dev", "tmat_cell_well_front_dev", "tmat_cell_area_fit_dev",
    "tmat_roi_sep_quads", "tmat_debug_sepconv_quads", "tmat_roi_sep_quads_pool", "tmat_debug_sepconv_pool_quads",
    "tmat_conv2d_narrow", "tmat_model_layers",
    "tmat_predict_smooth_ex", "tmat_smooth_plan", "tmat_spline_window", "tmat_smooth_begin", "tmat_smooth_tiles", "tmat_smooth_put",
    "tmat_smooth_end", "tmat_debug_smooth_times", "tmat_resize_pil_f32", "tmat_host_resize_pil_f32", "tmat_predict_auto_resample",
    "tmat_png_set_mode", "tmat_host_png_encode_batch_mode", "tmat_host_png_code_lengths", "tmat_debug_png_code_lengths",
    "tmat_tiff_probe", "tmat_host_tiff_decode_batch", "tmat_tiff_decode_batch", "tmat_tiff_decode_batch_dev",
    "tmat_tiff_decode_batch_dev_timed",
]

PIL_FILTERS = {"nearest": 0, "lanczos": 1}      # TMAT_PIL_*, Pillow's Image.Resampling numbers


def host_resize_pil_f32(x: np.ndarray, out_shape, resample: str) -> np.ndarray:
    """tmat_host_resize_pil_f32: PIL.Image.fromarray(x).resize(out_shape[::-1], resample) of float32 images (H, W) or (n, H, W) on the
    host; resample "lanczos" or "nearest"; out_shape (rows, cols)"""
    x = np.ascontiguousarray(x, np.float32)
    single = x.ndim == 2
    xb = x[None] if single else x
    out = np.empty((xb.shape[0], int(out_shape[0]), int(out_shape[1])), np.float32)
    check(lib().tmat_host_resize_pil_f32(ptr(xb), xb.shape[0], xb.shape[1], xb.shape[2], out.shape[1], out.shape[2], PIL_FILTERS[resample], ptr(out)),
          "tmat_host_resize_pil_f32")
    return out[0] if single else out


SMOOTH_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}       # TMAT_SMOOTH_*


def smooth_plan(hh: int, ww: int, window_size: int, subdivisions: int):
    """tmat_smooth_plan (include/tmat.h): (aug, step, (na, nb of the even frames, na, nb of the odd ones), n_tiles) of the smooth
    tiling of an hh x ww image.  Host only.  Raises TmatError (TMAT_E_ARG) for the geometries the stage refuses."""
    aug, step, n = C.c_int(0), C.c_int(0), C.c_int(0)
    counts = (C.c_int * 4)()
    check(lib().tmat_smooth_plan(int(hh), int(ww), int(window_size), int(subdivisions), C.byref(aug), C.byref(step), counts, C.byref(n)),
          "tmat_smooth_plan")
    return aug.value, step.value, tuple(counts), n.value


def spline_window(window_size: int) -> np.ndarray:
    """tmat_spline_window: smooth_tiled_predictions._spline_window(window_size) (reference :26-41), float64.  Host only."""
    win = np.empty(max(int(window_size), 0), np.float64)
    check(lib().tmat_spline_window(int(window_size), ptr(win)), "tmat_spline_window")
    return win


MODEL_LAUNCHERS = ("conv_mfma_kernel", "conv_narrow_kernel", "sepconv_ws_kernel")


def model_layers(weights_blob: bytes) -> np.ndarray:
    """tmat_model_layers (include/tmat.h): the convolution launches of one forward of a weight blob, in launch order, as an (n, 6) int32
    array of [ksize (2: sub-pixel form), stride, cin, cout, output side, launcher (index into MODEL_LAUNCHERS)].  Host only: no GPU, no
    handle.  Raises TmatError (TMAT_E_WEIGHTS, with the rule) for a blob whose filter counts no kernel takes."""
    L = lib()
    buf = (C.c_char * len(weights_blob)).from_buffer_copy(weights_blob)
    out = np.zeros((64, 6), np.int32)
    n = C.c_int(0)
    check(L.tmat_model_layers(C.cast(buf, C.c_void_p), len(weights_blob), out.shape[0], ptr(out), C.byref(n)), "tmat_model_layers")
    return out[:n.value].copy()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().tmat_last_error()
        raise TmatError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class VesselStages(C.Structure):
    """tmat_vessel_stages (include/tmat.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("vess", "sharp", "vessels", "edges", "skel", "mask_sel", "grown", "closed", "filt")]


class Handle:
    """Owns one tmat_handle (one HIP device + stream + resident weights)."""

    def __init__(self, weights_blob: "bytes | None", device_id: int = 0, max_patches: int = 0):
        """weights_blob None: a handle without a model (tmat_create_plain), enough for zproj / filter_edt / finish"""
        L = lib()
        self._h = C.c_void_p()
        self._blob = weights_blob
        if weights_blob is None:
            check(L.tmat_create_plain(device_id, C.byref(self._h)), "tmat_create_plain")
            return
        buf = (C.c_char * len(weights_blob)).from_buffer_copy(weights_blob)
        check(L.tmat_create(device_id, C.cast(buf, C.c_void_p), len(weights_blob), max_patches, C.byref(self._h)),
              "tmat_create")

    @property
    def raw(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().tmat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stage entry points --------------------------------------------------------------
    def unet_predict(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        check(lib().tmat_unet_predict(self._h, ptr(x), x.shape[0], ptr(y)), "tmat_unet_predict")
        return y

    def predict_smooth(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        single = x.ndim == 2
        xb = x[None] if single else x
        out = np.empty(xb.shape, np.float64)
        check(lib().tmat_predict_smooth(self._h, ptr(xb), xb.shape[0], xb.shape[1], xb.shape[2], ptr(out)),
              "tmat_predict_smooth")
        return out[0] if single else out

    def predict_smooth_ex(self, x: np.ndarray, subdivisions: int) -> np.ndarray:
        """tmat_predict_smooth_ex: predict_smooth for any subdivisions (2: predict_smooth itself)"""
        x = np.ascontiguousarray(x, np.float32)
        single = x.ndim == 2
        xb = x[None] if single else x
        out = np.empty(xb.shape, np.float64)
        check(lib().tmat_predict_smooth_ex(self._h, ptr(xb), xb.shape[0], xb.shape[1], xb.shape[2], int(subdivisions), ptr(out)),
              "tmat_predict_smooth_ex")
        return out[0] if single else out

    def resize_pil_f32(self, x: np.ndarray, out_shape, resample: str) -> np.ndarray:
        """tmat_resize_pil_f32: host_resize_pil_f32 on the device"""
        x = np.ascontiguousarray(x, np.float32)
        single = x.ndim == 2
        xb = x[None] if single else x
        out = np.empty((xb.shape[0], int(out_shape[0]), int(out_shape[1])), np.float32)
        check(lib().tmat_resize_pil_f32(self._h, ptr(xb), xb.shape[0], xb.shape[1], xb.shape[2], out.shape[1], out.shape[2], PIL_FILTERS[resample],
                                        ptr(out)), "tmat_resize_pil_f32")
        return out[0] if single else out

    def predict_auto_resample(self, x: np.ndarray, mid_shape, out_shape) -> np.ndarray:
        """tmat_predict_auto_resample: x (H, W) float32 -> LANCZOS to mid_shape (rows, cols) -> input norm -> smooth prediction ->
        float32 -> NEAREST to out_shape (rows, cols), one device chain"""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2:
            raise ValueError("predict_auto_resample: expected a 2-D single-channel image")
        out = np.empty((int(out_shape[0]), int(out_shape[1])), np.float32)
        check(lib().tmat_predict_auto_resample(self._h, ptr(x), x.shape[0], x.shape[1], int(mid_shape[0]), int(mid_shape[1]), out.shape[0], out.shape[1],
                                               ptr(out)), "tmat_predict_auto_resample")
        return out

    # smooth tiling around a predictor the caller runs (include/tmat.h: tmat_smooth_begin ... tmat_smooth_end)
    def smooth_begin(self, x: np.ndarray, window_size: int, subdivisions: int) -> int:
        """opens the session on x (hh, ww) float32 (a second begin discards an open one) -> n_tiles"""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2:
            raise ValueError("smooth_begin: expected a 2-D single-channel image")
        n = C.c_int(0)
        check(lib().tmat_smooth_begin(self._h, ptr(x), x.shape[0], x.shape[1], int(window_size), int(subdivisions), C.byref(n)),
              "tmat_smooth_begin")
        self._smooth_ws = int(window_size)
        return n.value

    def smooth_tiles(self, first: int, count: int) -> np.ndarray:
        """the tiles [first, first + count) of the open session, (count, ws, ws) float32"""
        ws = getattr(self, "_smooth_ws", 0)
        out = np.empty((max(int(count), 0), ws, ws), np.float32)
        check(lib().tmat_smooth_tiles(self._h, int(first), int(count), ptr(out)), "tmat_smooth_tiles")
        return out

    def smooth_put(self, first: int, preds: np.ndarray):
        """the predictor's results for the tiles [first, first + len(preds)): (k, ws, ws) or (k, ws, ws, 1), float32 or float64"""
        p = np.ascontiguousarray(preds)
        ws = getattr(self, "_smooth_ws", 0)
        if p.ndim == 4 and p.shape[-1] == 1:
            p = p.reshape(p.shape[:3])
        if p.dtype not in SMOOTH_DTYPES or p.ndim != 3 or p.shape[1:] != (ws, ws):
            raise ValueError(f"smooth_put: expected (k, {ws}, {ws}) float32 or float64 predictions")
        check(lib().tmat_smooth_put(self._h, int(first), p.shape[0], ptr(p), SMOOTH_DTYPES[p.dtype]), "tmat_smooth_put")

    def smooth_end(self, shape) -> np.ndarray:
        """blends what was put -> (hh, ww) float64 (shape: the image's); releases the session"""
        out = np.empty(tuple(shape), np.float64)
        check(lib().tmat_smooth_end(self._h, ptr(out)), "tmat_smooth_end")
        return out

    def smooth_times(self):
        """(tile gather ms, blend ms) on the device for the last session (tmat_debug_smooth_times)"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().tmat_debug_smooth_times(self._h, C.byref(a), C.byref(b)), "tmat_debug_smooth_times")
        return a.value, b.value

    def medial_axis(self, mask: np.ndarray):
        """tmat_medial_axis_batch: mask (n, h, w) bool/u8 -> (skel (n, h, w) bool, dist (n, h, w) f64), on the device"""
        m = np.ascontiguousarray(mask, np.uint8)
        skel = np.empty(m.shape, np.uint8)
        dist = np.empty(m.shape, np.float64)
        check(lib().tmat_medial_axis_batch(self._h, ptr(m), m.shape[0], m.shape[1], m.shape[2], ptr(skel), ptr(dist)), "tmat_medial_axis_batch")
        return skel.astype(bool), dist

    def filter_edt(self, pred: np.ndarray):
        """GPU binary morphology: pred (n, h, w) f64 -> (filtered mask bool, EDT f64)"""
        pred = np.ascontiguousarray(pred, np.float64)
        filt = np.empty(pred.shape, np.uint8)
        dist = np.empty(pred.shape, np.float64)
        check(lib().tmat_filter_edt_batch(self._h, ptr(pred), pred.shape[0], pred.shape[1], pred.shape[2], ptr(filt), ptr(dist)),
              "tmat_filter_edt_batch")
        return filt.astype(bool), dist

    def finish(self, pred, dist, skel, out_shape):
        """GPU: EDT(~skel), centre-line weighting, anti-aliased resize, rescale -> (field f32, field255 f32)"""
        pred = np.ascontiguousarray(pred, np.float64)
        dist = np.ascontiguousarray(dist, np.float64)
        skel = np.ascontiguousarray(np.asarray(skel) != 0, np.uint8)
        n = pred.shape[0]
        f = np.empty((n,) + tuple(out_shape), np.float32)
        f255 = np.empty_like(f)
        check(lib().tmat_finish_batch(self._h, ptr(pred), ptr(dist), ptr(skel), n, pred.shape[1], pred.shape[2], out_shape[0],
                                      out_shape[1], ptr(f), ptr(f255)), "tmat_finish_batch")
        return f, f255

    def filter_mask(self, masks, use_median=True, remove_isolated=True):
        """GPU filter_branch_seg_mask on (n, h, w) masks -> bool (n, h, w)"""
        m = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
        out = np.empty_like(m)
        check(lib().tmat_filter_mask_batch(self._h, ptr(m), m.shape[0], m.shape[1], m.shape[2], int(bool(use_median)),
                                           int(bool(remove_isolated)), ptr(out)), "tmat_filter_mask_batch")
        return out.astype(bool)

    def debug_filter_stages(self, masks, use_median=True, remove_isolated=True):
        """test-only: filter_mask with its stages (include/tmat.h:tmat_debug_filter_stages) on (n, h, w) masks -> dict of
        median, skeleton, filtered (n, h, w) u8, labels (n, h, w) i32, stats (n, 4, h, w) i32 (area, n1, n2, n3), thin_launches (n) i32"""
        m = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
        n = m.shape[0]
        out = {k: np.empty(m.shape, np.uint8) for k in ("median", "skeleton", "filtered")}
        out["labels"] = np.empty(m.shape, np.int32)
        out["stats"] = np.empty((n, 4) + m.shape[1:], np.int32)
        out["thin_launches"] = np.empty(n, np.int32)
        check(lib().tmat_debug_filter_stages(self._h, ptr(m), n, m.shape[1], m.shape[2], int(bool(use_median)), int(bool(remove_isolated)),
                                             *(ptr(out[k]) for k in ("median", "labels", "stats", "skeleton", "filtered", "thin_launches"))),
              "tmat_debug_filter_stages")
        return out

    def debug_medial_stages(self, masks):
        """test-only: medial_axis with the stages of its ordered thinning (include/tmat.h:tmat_debug_medial_stages) on (n, h, w) masks
        -> dict of skel, dep (n, h, w) u8, dist (n, h, w) f64, keys (n, h, w) u64, launches (1) i32"""
        m = np.ascontiguousarray(np.asarray(masks) != 0, np.uint8)
        out = {"skel": np.empty(m.shape, np.uint8), "dist": np.empty(m.shape, np.float64), "keys": np.empty(m.shape, np.uint64),
               "dep": np.empty(m.shape, np.uint8), "launches": np.zeros(1, np.int32)}
        check(lib().tmat_debug_medial_stages(self._h, ptr(m), m.shape[0], m.shape[1], m.shape[2],
                                             *(ptr(out[k]) for k in ("skel", "dist", "keys", "dep", "launches"))), "tmat_debug_medial_stages")
        return out

    ZPROJ_METHODS = {"fs": 0, "min": 1, "max": 2, "avg": 3, "med": 4}

    def zproj(self, stacks, method="fs"):
        """GPU Z projection of (n, Z, H, W) uint8/uint16 stacks -> (n, H, W); dtype as zstacks.py returns it
        (input dtype for fs / min / max, float64 for avg / med)"""
        stacks = np.asarray(stacks)
        if stacks.ndim != 4 or stacks.dtype not in (np.uint8, np.uint16):
            raise ValueError("zproj: expected (n, Z, H, W) uint8 or uint16 stacks")
        m = self.ZPROJ_METHODS[method]
        a = np.ascontiguousarray(stacks, np.uint16)
        n, Z, H, W = a.shape
        out = np.empty((n, H, W), np.float64 if m >= 3 else np.uint16)
        check(lib().tmat_zproj_batch(self._h, ptr(a), n, Z, H, W, m, ptr(out)), "tmat_zproj_batch")
        return out.astype(stacks.dtype) if m < 3 else out

    def zproj_dev(self, stacks_dev, shape, method="fs", dtype=np.uint16):
        """tmat_zproj_dev: the same for (n, Z, H, W) uint16 stacks resident in a tmat_dev_alloc block (8-bit sources widened: pass
        dtype=np.uint8 to get fs / min / max back as zproj returns them)"""
        m = self.ZPROJ_METHODS[method]
        n, Z, H, W = (int(v) for v in shape)
        out = np.empty((n, H, W), np.float64 if m >= 3 else np.uint16)
        d = C.c_void_p()
        check(lib().tmat_dev_alloc(self._h, max(out.nbytes, 1), C.byref(d)), "tmat_dev_alloc")
        try:
            check(lib().tmat_zproj_dev(self._h, stacks_dev, n, Z, H, W, m, d), "tmat_zproj_dev")
            check(lib().tmat_dev_download(self._h, ptr(out), d, out.nbytes), "tmat_dev_download")
        finally:
            lib().tmat_dev_free(self._h, d)
        return out.astype(dtype) if m < 3 else out

    def set_input_norm(self, norm_mean=None, norm_std=None):
        """models.py:636-637 on the device: x = (x - norm_mean) / norm_std in front of the smooth prediction; None turns it off"""
        on = norm_mean is not None and norm_std is not None
        check(lib().tmat_set_input_norm(self._h, int(on), float(norm_mean or 0.0), float(norm_std if on else 1.0)), "tmat_set_input_norm")

    def set_precision(self, mode="f32"):
        """arithmetic of the UNet's dense convolutions: "f32" (bit-exact contract, default) "bf16x3" or "bf16x6" (opt-in split
        precision on the bf16 matrix cores, include/tmat.h:tmat_set_precision)"""
        modes = {"f32": 0, "bf16x3": 1, "bf16x6": 2}
        if mode not in modes:
            raise ValueError(f"precision must be one of {sorted(modes)}")
        check(lib().tmat_set_precision(self._h, modes[mode]), "tmat_set_precision")

    def resnet_set_precision(self, mode="f32"):
        """arithmetic of the invasion-depth classifiers' convolutions: "f32" (bit-exact contract, default), "f16" (opt-in: operands
        rounded to IEEE f16, f32 accumulation on the f16 matrix cores) or "f16act" (opt-in: the f16 mode with every activation tensor
        stored as IEEE f16; include/tmat.h:tmat_resnet_set_precision)"""
        modes = {"f32": 0, "f16": 1, "f16act": 3}
        if mode not in modes:
            raise ValueError(f"precision must be one of {sorted(modes)}")
        check(lib().tmat_resnet_set_precision(self._h, modes[mode]), "tmat_resnet_set_precision")

    def conv2d(self, x, w, scale, shift, stride=1, resid=None, relu_in=False, relu_out=False, prec=0):
        """stage-wise test entry point (include/tmat.h:tmat_conv2d): one convolution of the MFMA kernel.  x (n, h, w, cin), w in the Keras
        layout (k, k, cin, cout), scale (nullable) / shift (cout), resid (nullable) shaped like the result; prec 0 (f32), 3 (f16 operands) or
        4 (one f16act convolution: x and resid rounded to f16, f16 buffers on the device, the f16 result widened)"""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        n, hh, ww, cin = x.shape
        k, k2, ci2, cout = w.shape
        if k != k2 or ci2 != cin:
            raise ValueError("conv2d: weight shape does not match the input")
        shift = np.ascontiguousarray(shift, np.float32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
        out = np.empty((n, hh // stride, ww // stride, cout), np.float32)
        if resid is not None:
            resid = np.ascontiguousarray(resid, np.float32)
            if resid.shape != out.shape:
                raise ValueError("conv2d: resid must have the shape of the result")
        if shift.shape != (cout,) or (scale is not None and scale.shape != (cout,)):
            raise ValueError("conv2d: scale / shift must have cout entries")
        check(lib().tmat_conv2d(self._h, int(prec), ptr(x), n, hh, ww, cin, ptr(w), k, int(stride), cout, None if scale is None else ptr(scale), ptr(shift),
                                None if resid is None else ptr(resid), int(bool(relu_in)), int(bool(relu_out)), ptr(out)), "tmat_conv2d")
        return out

    def conv2d_roi(self, x, w, scale, shift, segs, out, resid=None, rs=0, subpixel=False, relu_in=False, relu_out=False, out_relu=None):
        """stage-wise test entry point of the region form (include/tmat.h:tmat_conv2d_roi): one f32 convolution of the MFMA kernel with a
        segment table.  x (n, h, w, cin), w in the Keras layout (k, k, cin, cout); segs: at most 64 rows (p0, np, y0, x0, rh, rw; a patch range may repeat with disjoint rectangles), none for
        the full-frame launch; resid (nullable) (n, h >> rs, w >> rs, cout); subpixel: the 3x3 over the 2x nearest-upsampled x, out
        (n, 2 h, 2 w, cout), segments in stored pixels.  out (and out_relu, nullable) are caller-filled float32 arrays, changed in place:
        words outside the rectangles keep their value.  Returns out."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        n, hh, ww, cin = x.shape
        k, k2, ci2, cout = w.shape
        if k != k2 or ci2 != cin:
            raise ValueError("conv2d_roi: weight shape does not match the input")
        up = 2 if subpixel else 1
        for o in (out, out_relu):
            if o is not None and (o.dtype != np.float32 or not o.flags.c_contiguous or o.shape != (n, hh * up, ww * up, cout)):
                raise ValueError("conv2d_roi: out / out_relu must be C-contiguous float32 arrays of the result's shape")
        shift = np.ascontiguousarray(shift, np.float32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
        if resid is not None:
            resid = np.ascontiguousarray(resid, np.float32)
            if resid.shape != (n, hh >> rs, ww >> rs, cout):
                raise ValueError("conv2d_roi: resid must be (n, h >> rs, w >> rs, cout)")
        if shift.shape != (cout,) or (scale is not None and scale.shape != (cout,)):
            raise ValueError("conv2d_roi: scale / shift must have cout entries")
        sg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 6))
        check(lib().tmat_conv2d_roi(self._h, ptr(x), n, hh, ww, cin, ptr(w), k, int(bool(subpixel)), cout, None if scale is None else ptr(scale),
                                    ptr(shift), None if resid is None else ptr(resid), int(rs), int(bool(relu_in)), int(bool(relu_out)),
                                    ptr(sg) if len(sg) else None, len(sg), ptr(out), None if out_relu is None else ptr(out_relu)), "tmat_conv2d_roi")
        return out

    def conv2d_roi_s2(self, x, w, scale, shift, segs, out, relu_in=False, relu_out=False, out_relu=None):
        """conv2d_roi for the 1x1 form at stride 2 (include/tmat.h:tmat_conv2d_roi_s2): x (n, h, w, cin) with even h and w, w (1, 1, cin, cout),
        out (and out_relu, nullable) caller-filled (n, h / 2, w / 2, cout), segs in output pixels.  Returns out."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        n, hh, ww, cin = x.shape
        if w.shape[:3] != (1, 1, cin) or (hh | ww) & 1:
            raise ValueError("conv2d_roi_s2: w must be (1, 1, cin, cout), h and w even")
        cout = w.shape[3]
        for o in (out, out_relu):
            if o is not None and (o.dtype != np.float32 or not o.flags.c_contiguous or o.shape != (n, hh // 2, ww // 2, cout)):
                raise ValueError("conv2d_roi_s2: out / out_relu must be C-contiguous float32 arrays of the result's shape")
        shift = np.ascontiguousarray(shift, np.float32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
        if shift.shape != (cout,) or (scale is not None and scale.shape != (cout,)):
            raise ValueError("conv2d_roi_s2: scale / shift must have cout entries")
        sg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 6))
        L = lib()
        L.tmat_conv2d_roi_s2.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
        check(L.tmat_conv2d_roi_s2(self._h, ptr(x), n, hh, ww, cin, ptr(w), cout, None if scale is None else ptr(scale), ptr(shift),
                                   int(bool(relu_in)), int(bool(relu_out)), ptr(sg) if len(sg) else None, len(sg), ptr(out),
                                   None if out_relu is None else ptr(out_relu)), "tmat_conv2d_roi_s2")
        return out

    def conv2d_narrow(self, x, w, scale, shift, segs, out, stride=1, resid=None, rs=0, subpixel=False, relu_in=False, relu_out=False, out_relu=None):
        """conv2d_roi on the narrow layers' kernel (include/tmat.h:tmat_conv2d_narrow): cin and cout multiples of 16, stride 1 or 2 (ksize 1).
        out (and out_relu, nullable) caller-filled (n, h up / stride, w up / stride, cout), up = 2 for the sub-pixel form; segs none for the
        full-frame launch.  Returns out."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        n, hh, ww, cin = x.shape
        k, k2, ci2, cout = w.shape
        if k != k2 or ci2 != cin:
            raise ValueError("conv2d_narrow: weight shape does not match the input")
        up = 2 if subpixel else 1
        for o in (out, out_relu):
            if o is not None and (o.dtype != np.float32 or not o.flags.c_contiguous or o.shape != (n, hh * up // stride, ww * up // stride, cout)):
                raise ValueError("conv2d_narrow: out / out_relu must be C-contiguous float32 arrays of the result's shape")
        shift = np.ascontiguousarray(shift, np.float32)
        scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
        if resid is not None:
            resid = np.ascontiguousarray(resid, np.float32)
            if resid.shape != (n, hh >> rs, ww >> rs, cout):
                raise ValueError("conv2d_narrow: resid must be (n, h >> rs, w >> rs, cout)")
        if shift.shape != (cout,) or (scale is not None and scale.shape != (cout,)):
            raise ValueError("conv2d_narrow: scale / shift must have cout entries")
        sg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 6))
        check(lib().tmat_conv2d_narrow(self._h, ptr(x), n, hh, ww, cin, ptr(w), k, int(stride), int(bool(subpixel)), cout,
                                       None if scale is None else ptr(scale), ptr(shift), None if resid is None else ptr(resid), int(rs),
                                       int(bool(relu_in)), int(bool(relu_out)), ptr(sg) if len(sg) else None, len(sg), ptr(out),
                                       None if out_relu is None else ptr(out_relu)), "tmat_conv2d_narrow")
        return out

    def render_tree(self, backgrounds, trees, vis_width=2000):
        """tmat_render_tree: the tree overlays of n backgrounds (n, bh, bw) u16 / f32 on the device -> (n, vh, vw, 3) u8;
        trees: one (segs (k, 4) f64, seg_branch (k) i32) pair per image, as morse_tree returns them"""
        bg, dt, segs, sb, off, out = _render_tree_args(backgrounds, trees, vis_width)
        check(lib().tmat_render_tree(self._h, ptr(bg), dt, bg.shape[0], bg.shape[1], bg.shape[2], ptr(segs), ptr(sb), ptr(off), int(vis_width),
                                     ptr(out)), "tmat_render_tree")
        return out

    def render_tree_timed(self, backgrounds, trees, vis_width=2000):
        """tmat_render_tree_timed: (overlays, {phase: HIP-event ms}) with the phases upload, minmax, render, copy_back"""
        bg, dt, segs, sb, off, out = _render_tree_args(backgrounds, trees, vis_width)
        ms = np.zeros(4, np.float32)
        check(lib().tmat_render_tree_timed(self._h, ptr(bg), dt, bg.shape[0], bg.shape[1], bg.shape[2], ptr(segs), ptr(sb), ptr(off), int(vis_width),
                                           ptr(out), ptr(ms)), "tmat_render_tree_timed")
        return out, dict(zip(("upload", "minmax", "render", "copy_back"), (float(v) for v in ms)))

    def stage_pictures(self, a):
        """tmat_stage_pictures: save_vis of (n, ...) images u16 / f32 / f64 / u8 (bool counts as u8) on the device -> u8 of the same shape;
        a 2-D array is one image"""
        a, shape = _stage_pictures_arg(a)
        out = np.empty(a.shape, np.uint8)
        if a.shape[0]:
            check(lib().tmat_stage_pictures(self._h, ptr(a), PIC_DTYPES[a.dtype], a.shape[0], a[0].size, ptr(out)), "tmat_stage_pictures")
        return out.reshape(shape)

    def png_set_mode(self, mode="fast"):
        """tmat_png_set_mode: "fast" (the default) or "compact" (lazy parse, dynamic Huffman blocks: smaller files) for every PNG file the
        handle encodes from now on"""
        check(lib().tmat_png_set_mode(self._h, _png_mode(mode)), "tmat_png_set_mode")

    def debug_png_code_lengths(self, freqs, limit):
        """tmat_debug_png_code_lengths: (k, n) histograms -> (k, n) u8 code lengths, computed on the device"""
        f = np.ascontiguousarray(freqs, np.uint32)
        lens = np.zeros(f.shape, np.uint8)
        check(lib().tmat_debug_png_code_lengths(self._h, ptr(f), f.shape[0], f.shape[1], int(limit), ptr(lens)), "tmat_debug_png_code_lengths")
        return lens

    def png_encode(self, pics):
        """tmat_png_encode_batch: (n, H, W) grey or (n, H, W, 3) RGB u8 pictures -> n PNG files (bytes), encoded on the device; a 2-D or
        (H, W, 3) array is one picture"""
        pics = _png_arg(pics)
        return _png_call(lambda *a: lib().tmat_png_encode_batch(self._h, *a), pics, "tmat_png_encode_batch")

    def png_encode_dev(self, pics_dev, n, H, W, channels):
        """tmat_png_encode_batch_dev: the same for n pictures already in device memory (a tmat_dev_alloc pointer)"""
        return _png_call(lambda _, *a: lib().tmat_png_encode_batch_dev(self._h, pics_dev, *a), (n, H, W, channels), "tmat_png_encode_batch_dev")

    def png_encode_timed(self, pics):
        """tmat_png_encode_batch_timed: (files, {phase: HIP-event ms}) with the phases upload, kernels, copy_back"""
        pics = _png_arg(pics)
        ms = np.zeros(3, np.float32)
        files = _png_call(lambda *a: lib().tmat_png_encode_batch_timed(self._h, *a, ptr(ms)), pics, "tmat_png_encode_batch_timed")
        return files, dict(zip(("upload", "kernels", "copy_back"), (float(v) for v in ms)))

    def tiff_decode(self, files, planes, H, W, out=None):
        """tmat_tiff_decode_batch: planes (a list of (file index, page)) of the TIFF files (a list of bytes), decoded on the device ->
        (pixels (n, H, W) uint16, bits, status (n,)); planes whose status is not TIFF_OK keep what `out` held (zeros without one)"""
        if out is None:
            out = np.zeros((len(planes), int(H), int(W)), np.uint16)
        assert out.dtype == np.uint16 and out.flags.c_contiguous and out.shape == (len(planes), int(H), int(W))
        bits, status = _tiff_call(lambda *a: lib().tmat_tiff_decode_batch(self._h, *a), files, planes, H, W, ptr(out), "tmat_tiff_decode_batch")
        return out, bits, status

    def tiff_decode_dev(self, files, planes, H, W, out_dev):
        """tmat_tiff_decode_batch_dev: the same into out_dev, a tmat_dev_alloc block of n H W uint16 -> (bits, status (n,))"""
        return _tiff_call(lambda *a: lib().tmat_tiff_decode_batch_dev(self._h, *a), files, planes, H, W, out_dev, "tmat_tiff_decode_batch_dev")

    def tiff_decode_dev_timed(self, files, planes, H, W, out_dev):
        """tmat_tiff_decode_batch_dev_timed: (bits, status, {phase: HIP-event ms}) with the phases upload and kernels"""
        ms = np.zeros(2, np.float32)
        bits, status = _tiff_call(lambda *a: lib().tmat_tiff_decode_batch_dev_timed(self._h, *a, ptr(ms)), files, planes, H, W, out_dev,
                                  "tmat_tiff_decode_batch_dev_timed")
        return bits, status, dict(upload=float(ms[0]), kernels=float(ms[1]))

    def render_tree_png(self, backgrounds, trees, vis_width=2000):
        """tmat_render_tree_png: Handle.render_tree's overlays as n PNG files (bytes); the raw overlays stay on the device"""
        bg, dt, segs, sb, off, _ = _render_tree_args(backgrounds, trees, vis_width, want_out=False)
        vh, vw = tree_canvas_shape(bg.shape[1], bg.shape[2], vis_width)
        return _png_call(lambda _, n, H, W, ch, *a: lib().tmat_render_tree_png(self._h, ptr(bg), dt, n, bg.shape[1], bg.shape[2], ptr(segs), ptr(sb),
                                                                                ptr(off), int(vis_width), *a),
                         (bg.shape[0], vh, vw, 3), "tmat_render_tree_png")

    def render_barcode(self, bars_list, vis_width=2000):
        """tmat_render_barcode: the barcode pictures of a batch on the device -> (n, S, S, 3) u8; bars_list: one (k, 2) f64 array per picture"""
        bars, off = _barcode_args(bars_list)
        S = int(round(vis_width * 0.9))
        out = np.empty((len(bars_list), S, S, 3), np.uint8)
        check(lib().tmat_render_barcode(self._h, ptr(bars), ptr(off), len(bars_list), int(vis_width), ptr(out)), "tmat_render_barcode")
        return out

    def render_barcode_png(self, bars_list, vis_width=2000):
        """tmat_render_barcode_png: Handle.render_barcode's pictures as PNG files (bytes); the canvases stay on the device"""
        bars, off = _barcode_args(bars_list)
        S = int(round(vis_width * 0.9))
        return _png_call(lambda _, n, H, W, ch, *a: lib().tmat_render_barcode_png(self._h, ptr(bars), ptr(off), n, int(vis_width), *a),
                         (len(bars_list), S, S, 3), "tmat_render_barcode_png")

    def debug_poison(self, byte_pattern=0xFF):
        """test-only: fill every scratch workspace of the handle with a byte pattern (include/tmat.h:tmat_debug_poison)"""
        check(lib().tmat_debug_poison(self._h, int(byte_pattern)), "tmat_debug_poison")

    def debug_sep_tiles(self):
        """test-only: [(planned tiles, full-frame tiles)] of the fused separable launches of the last down pass (include/tmat.h:tmat_debug_sep_tiles)"""
        L = lib()
        L.tmat_debug_sep_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        n = np.zeros(1, np.int32)
        planned, full = np.zeros(16, np.int64), np.zeros(16, np.int64)
        check(L.tmat_debug_sep_tiles(self._h, 16, ptr(n), ptr(planned), ptr(full)), "tmat_debug_sep_tiles")
        return [(int(planned[i]), int(full[i])) for i in range(min(int(n[0]), 16))]

    def debug_sepconv_quads(self, x, dw9, pw, scale, shift, quads, out, relu_in=False, relu_out=True, stem=None):
        """test-only (include/tmat.h:tmat_debug_sepconv_quads): one plain fused separable launch in quadrant form.  x (n, h, w, cin), or
        with stem = (taps [9][cin], scale, shift) the single-channel patches (n, 2 h, 2 w); dw9 [9][cin]; pw (cin, cout) in the Keras layout;
        quads: full-frame quadrant ids; out (n, h, w, cout) float32, caller-filled, changed in place and returned."""
        x, dw9, pw = (np.ascontiguousarray(a, np.float32) for a in (x, dw9, pw))
        scale, shift = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(shift, np.float32)
        q = np.ascontiguousarray(quads, np.int32).ravel()
        cin, cout = pw.shape
        n, hh, ww = out.shape[:3]
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (n, hh, ww, cout) and dw9.shape == (9, cin)
        assert x.shape == ((n, 2 * hh, 2 * ww) if stem is not None else (n, hh, ww, cin)), x.shape
        st = [None] * 3 if stem is None else [np.ascontiguousarray(a, np.float32) for a in stem]
        assert stem is None or (st[0].shape == (9, cin) and st[1].shape == (cin,) and st[2].shape == (cin,))
        L = lib()
        vp, i = C.c_void_p, C.c_int
        L.tmat_debug_sepconv_quads.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, i, vp]
        check(L.tmat_debug_sepconv_quads(self._h, ptr(x), n, hh, ww, cin, int(bool(relu_in)), ptr(dw9), ptr(pw), cout, ptr(scale), ptr(shift),
                                         int(bool(relu_out)), *(None if a is None else ptr(a) for a in st), ptr(q), len(q), ptr(out)),
              "tmat_debug_sepconv_quads")
        return out

    def debug_sepconv_pool_quads(self, x, dw9, pw, scale, shift, resid, quads, out, relu_in=False, relu_out=False):
        """test-only (include/tmat.h:tmat_debug_sepconv_pool_quads): one pooled fused separable launch in quadrant form and its fix-up.
        x (n, h, w, cin); dw9 [9][cin]; pw (cin, cout) in the Keras layout; resid and out (n, h / 2, w / 2, cout) float32; quads: full-frame
        quadrant ids; out is caller-filled, changed in place and returned."""
        x, dw9, pw, resid = (np.ascontiguousarray(a, np.float32) for a in (x, dw9, pw, resid))
        scale, shift = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(shift, np.float32)
        q = np.ascontiguousarray(quads, np.int32).ravel()
        cin, cout = pw.shape
        n, hh, ww = x.shape[:3]
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (n, hh // 2, ww // 2, cout) and dw9.shape == (9, cin)
        assert x.shape == (n, hh, ww, cin) and resid.shape == out.shape
        L = lib()
        vp, i = C.c_void_p, C.c_int
        L.tmat_debug_sepconv_pool_quads.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, vp, vp, i, vp, vp, i, vp]
        check(L.tmat_debug_sepconv_pool_quads(self._h, ptr(x), n, hh, ww, cin, int(bool(relu_in)), ptr(dw9), ptr(pw), cout, ptr(scale), ptr(shift),
                                              int(bool(relu_out)), ptr(resid), ptr(q), len(q), ptr(out)), "tmat_debug_sepconv_pool_quads")
        return out

    def debug_down_segs(self):
        """test-only: the longest segment table among the rectangle launches of the last down pass (include/tmat.h:tmat_debug_down_segs)"""
        n = C.c_int()
        check(lib().tmat_debug_down_segs(self._h, C.byref(n)), "tmat_debug_down_segs")
        return n.value

    def debug_down_seg_total(self):
        """test-only: the segments of all rectangle launches of the last down pass together (include/tmat.h:tmat_debug_down_seg_total)"""
        n = C.c_int()
        check(lib().tmat_debug_down_seg_total(self._h, C.byref(n)), "tmat_debug_down_seg_total")
        return n.value

    def debug_held_bytes(self):
        """test-only: (device bytes, pinned bytes) the handle retains between calls (include/tmat.h:tmat_debug_held_bytes)"""
        dev, pin = C.c_size_t(), C.c_size_t()
        check(lib().tmat_debug_held_bytes(self._h, C.byref(dev), C.byref(pin)), "tmat_debug_held_bytes")
        return dev.value, pin.value

    def prof_enable(self, on=True):
        check(lib().tmat_prof_enable(self._h, int(on)), "tmat_prof_enable")

    def prof_read(self, reset=True):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        check(lib().tmat_prof_read(self._h, C.byref(ms), C.byref(n), C.byref(fl), int(reset)), "tmat_prof_read")
        return ms.value, n.value, fl.value


# -- host-only entry points (no handle / no GPU needed) ------------------------------------------
def dmt_graph(img: np.ndarray, delta1: float, delta2: float = 0.0, handle: "Handle | None" = None):
    """tmat_dmt_graph: (vertices (n,2) int32 [row, col], edges (m,2) int32)."""
    img = np.ascontiguousarray(img, np.float32)
    R, Cc = img.shape
    cap_v, cap_e = R * Cc + 4, 3 * R * Cc + 4
    V = np.empty((cap_v, 2), np.int32)
    E = np.empty((cap_e, 2), np.int32)
    nv, ne = C.c_int(), C.c_int()
    check(lib().tmat_dmt_graph(handle.raw if handle else None, ptr(img), R, Cc, float(delta1), float(delta2), ptr(V), cap_v,
                               ptr(E), cap_e, C.byref(nv), C.byref(ne)), "tmat_dmt_graph")
    return V[: nv.value].copy(), E[: ne.value].copy()


def dmt_graph_batch(imgs: np.ndarray, delta1: float, delta2: float = 0.0, handle: "Handle | None" = None):
    """tmat_dmt_graph_batch: n fields of one shape in one call -> list of (vertices, edges) as dmt_graph returns them."""
    imgs = np.ascontiguousarray(imgs, np.float32)
    n, R, Cc = imgs.shape
    cap_v, cap_e = R * Cc + 4, 3 * R * Cc + 4
    V = np.empty((n, cap_v, 2), np.int32)
    E = np.empty((n, cap_e, 2), np.int32)
    nv, ne = np.zeros(n, np.int32), np.zeros(n, np.int32)
    check(lib().tmat_dmt_graph_batch(handle.raw if handle else None, ptr(imgs), n, R, Cc, float(delta1), float(delta2), ptr(V), cap_v,
                                     ptr(E), cap_e, ptr(nv), ptr(ne)), "tmat_dmt_graph_batch")
    return [(V[k, : nv[k]].copy(), E[k, : ne[k]].copy()) for k in range(n)]


def morse_stats(V, E, shape, smoothing_window, min_branch_length, max_branch_length=None,
                remove_isolated_branches=False, pruning_mask=None):
    """tmat_morse_stats: (bars (k,2) f64, count, total_px, avg_px)."""
    V = np.ascontiguousarray(V, np.int32).reshape(-1, 2)
    E = np.ascontiguousarray(E, np.int32).reshape(-1, 2)
    pm = None
    if pruning_mask is not None:
        pm = np.ascontiguousarray(np.asarray(pruning_mask) > 0, np.uint8)
    cap = max(len(V), 1)
    bars = np.empty((cap, 2), np.float64)
    cnt, tot, avg = C.c_int64(), C.c_double(), C.c_double()
    check(lib().tmat_morse_stats(ptr(V), len(V), ptr(E), len(E), int(shape[0]), int(shape[1]), int(smoothing_window),
                                 int(min_branch_length), int(max_branch_length or 0), int(bool(remove_isolated_branches)),
                                 ptr(pm) if pm is not None else None, C.byref(cnt), C.byref(tot), C.byref(avg), ptr(bars), cap),
          "tmat_morse_stats")
    return bars[: cnt.value].copy(), cnt.value, tot.value, avg.value


def morse_tree(V, E, shape, smoothing_window, min_branch_length, max_branch_length=None, remove_isolated_branches=False,
               pruning_mask=None, scaling_factor=1.0):
    """tmat_morse_tree: (segs (s, 4) f64 [x1, y1, x2, y2], seg_branch (s) i32, bars (k, 2) f64 scaled, count, total_px, avg_px)."""
    V = np.ascontiguousarray(V, np.int32).reshape(-1, 2)
    E = np.ascontiguousarray(E, np.int32).reshape(-1, 2)
    pm = None
    if pruning_mask is not None:
        pm = np.ascontiguousarray(np.asarray(pruning_mask) > 0, np.uint8)
    cap = max(len(V), 1)                      # a forest has fewer edges than vertices, and every segment is one of its edges
    segs = np.empty((cap, 4), np.float64)
    sb = np.empty(cap, np.int32)
    bars = np.empty((cap, 2), np.float64)
    cnt, tot, avg, ns, nb = C.c_int64(), C.c_double(), C.c_double(), C.c_int(), C.c_int()
    check(lib().tmat_morse_tree(ptr(V), len(V), ptr(E), len(E), int(shape[0]), int(shape[1]), int(smoothing_window),
                                int(min_branch_length), int(max_branch_length or 0), int(bool(remove_isolated_branches)),
                                ptr(pm) if pm is not None else None, float(scaling_factor), C.byref(cnt), C.byref(tot), C.byref(avg),
                                ptr(segs), ptr(sb), cap, ptr(bars), cap, C.byref(ns), C.byref(nb)), "tmat_morse_tree")
    return segs[: ns.value].copy(), sb[: ns.value].copy(), bars[: nb.value].copy(), cnt.value, tot.value, avg.value


def branch_color(i):
    """tmat_branch_color: the (R, G, B) bytes branch i is drawn in"""
    rgb = np.zeros(3, np.uint8)
    check(lib().tmat_branch_color(int(i), ptr(rgb)), "tmat_branch_color")
    return rgb


def tree_canvas_shape(bh, bw, vis_width=2000):
    """(vh, vw) of the overlay of a (bh, bw) background: Python's round() is round-half-even, as the library's"""
    return int(round(vis_width * bh / bw)), int(vis_width)


def _render_tree_args(backgrounds, trees, vis_width, want_out=True):
    bg = np.asarray(backgrounds)
    if bg.ndim == 2:
        bg = bg[None]
    if bg.ndim != 3 or len(trees) != bg.shape[0]:
        raise ValueError("render_tree: expected (n, bh, bw) backgrounds and one (segs, seg_branch) pair per image")
    bg = np.ascontiguousarray(bg, np.uint16 if bg.dtype == np.uint16 else np.float32)
    off = np.zeros(len(trees) + 1, np.int32)
    off[1:] = np.cumsum([len(t[0]) for t in trees])
    segs = np.ascontiguousarray(np.concatenate([np.asarray(t[0], np.float64).reshape(-1, 4) for t in trees] + [np.zeros((1, 4))]))
    sb = np.ascontiguousarray(np.concatenate([np.asarray(t[1], np.int32).reshape(-1) for t in trees] + [np.zeros(1, np.int32)]))
    vh, vw = tree_canvas_shape(bg.shape[1], bg.shape[2], vis_width)
    out = np.empty((bg.shape[0], vh, vw, 3), np.uint8) if want_out else None
    return bg, 0 if bg.dtype == np.uint16 else 1, segs, sb, off, out


def host_render_tree(backgrounds, trees, vis_width=2000):
    """tmat_host_render_tree: the host twin of Handle.render_tree (same bytes, no GPU)"""
    bg, dt, segs, sb, off, out = _render_tree_args(backgrounds, trees, vis_width)
    check(lib().tmat_host_render_tree(ptr(bg), dt, bg.shape[0], bg.shape[1], bg.shape[2], ptr(segs), ptr(sb), ptr(off), int(vis_width), ptr(out)),
          "tmat_host_render_tree")
    return out


def png_stripe():
    """tmat_png_stripe: bytes of filtered stream one stripe of the PNG encoder compresses"""
    return int(lib().tmat_png_stripe())


def png_bound(H, W, channels):
    """tmat_png_bound: the worst-case size of one file"""
    b = C.c_size_t()
    check(lib().tmat_png_bound(int(H), int(W), int(channels), C.byref(b)), "tmat_png_bound")
    return int(b.value)


def _png_arg(pics):
    a = np.asarray(pics)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError(f"png_encode: expected uint8 pictures, got {a.dtype}")
    if a.ndim == 2 or (a.ndim == 3 and a.shape[-1] == 3):       # one grey picture; a 3-D array whose last axis is 3 is one RGB picture
        a = a[None]
    if a.ndim not in (3, 4) or (a.ndim == 4 and a.shape[3] != 3):
        raise ValueError(f"png_encode: expected (n, H, W) or (n, H, W, 3) pictures, got {a.shape}")
    return np.ascontiguousarray(a)


def _png_call(fn, pics, what):
    """fn(pics pointer, n, H, W, channels, out, cap_each, sizes) -> the n files; pics: an array, or (n, H, W, channels) for a call that brings its own"""
    if isinstance(pics, tuple):
        n, H, W, ch = (int(v) for v in pics)
        src = None
    else:
        n, H, W = pics.shape[:3]
        ch = 3 if pics.ndim == 4 else 1
        src = ptr(pics)
    cap = png_bound(H, W, ch)
    out = np.empty((n, cap), np.uint8)
    sizes = np.zeros(max(n, 1), np.uintp)
    check(fn(src, n, H, W, ch, ptr(out), cap, ptr(sizes)), what)
    return [out[i, : int(sizes[i])].tobytes() for i in range(n)]


PNG_MODES = {"fast": 0, "compact": 1}       # TMAT_PNG_FAST, TMAT_PNG_COMPACT


def _png_mode(mode):
    if mode not in PNG_MODES:
        raise ValueError(f"png mode must be one of {sorted(PNG_MODES)}")
    return PNG_MODES[mode]


def host_png_encode(pics, mode="fast"):
    """tmat_host_png_encode_batch_mode: the host twin of Handle.png_encode in the given mode (same bytes, no GPU)"""
    m = _png_mode(mode)
    return _png_call(lambda *a: lib().tmat_host_png_encode_batch_mode(*a, m), _png_arg(pics), "tmat_host_png_encode_batch_mode")


def host_png_code_lengths(freq, limit):
    """tmat_host_png_code_lengths: a histogram (n) -> its code lengths (n) u8"""
    f = np.ascontiguousarray(freq, np.uint32)
    lens = np.zeros(f.shape, np.uint8)
    check(lib().tmat_host_png_code_lengths(ptr(f), f.shape[0], int(limit), ptr(lens)), "tmat_host_png_code_lengths")
    return lens


TIFF_OK, TIFF_FALLBACK, TIFF_CORRUPT = 0, 1, 2          # TMAT_TIFF_OK, TMAT_TIFF_FALLBACK, TMAT_TIFF_CORRUPT
TIFF_REASONS = {0: "none", 1: "header", 2: "ifd", 3: "loop", 4: "tag", 5: "strips", 6: "stream", 7: "page", 20: "bigtiff", 21: "tiles",
                22: "samples", 23: "bits", 24: "sample_format", 25: "photometric", 26: "fill_order", 27: "planar", 28: "compression",
                29: "predictor", 30: "old_lzw", 31: "size"}                                     # TMAT_TIFF_R_*
TIFF_PAGE_FIELDS = ("width", "height", "bits", "compression", "predictor", "big_endian", "rows_per_strip", "n_strips", "status", "reason")


def tiff_probe(data: bytes):
    """tmat_tiff_probe: the pages of a TIFF file held in memory, one dict per page with the fields of tmat_tiff_page (`reason` as its
    name in TIFF_REASONS).  Host only: no GPU, no handle.  A damaged header or IFD chain ends the list with a page of status TIFF_CORRUPT."""
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    n, cap = C.c_int(0), 16
    while True:
        pages = np.zeros((cap, len(TIFF_PAGE_FIELDS)), np.int32)
        check(lib().tmat_tiff_probe(ptr(buf), len(data), cap, ptr(pages), C.byref(n)), "tmat_tiff_probe")
        if n.value <= cap:
            break
        cap = n.value
    out = [dict(zip(TIFF_PAGE_FIELDS, (int(v) for v in row))) for row in pages[: n.value]]
    for p in out:
        p["reason"] = TIFF_REASONS.get(p["reason"], str(p["reason"]))
    return out


def _tiff_call(fn, files, planes, H, W, out, what):
    """fn(files, n_bytes, file_of, page_of, n_planes, H, W, out, bits, status) over files (a list of bytes) and planes (a list of
    (file index, page)) -> (bits, status (n_planes,) int32)"""
    bufs = [np.frombuffer(f, np.uint8) if len(f) else np.zeros(1, np.uint8) for f in files]
    for fi, pg in planes:
        if not 0 <= int(fi) < len(files):
            raise ValueError(f"{what}: file index {fi} outside the {len(files)} files")
    fptr = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs])
    nb = np.array([len(f) for f in files] or [0], np.uintp)
    fo = np.array([int(p[0]) for p in planes] or [0], np.int32)
    po = np.array([int(p[1]) for p in planes] or [0], np.int32)
    status = np.zeros(max(len(planes), 1), np.int32)
    bits = C.c_int(0)
    check(fn(C.cast(fptr, C.c_void_p), ptr(nb), ptr(fo), ptr(po), len(planes), int(H), int(W), out, C.byref(bits), ptr(status)), what)
    return bits.value, status[: len(planes)]


def host_tiff_decode(files, planes, H, W, out=None):
    """tmat_host_tiff_decode_batch: the host twin of Handle.tiff_decode (same pixels and status, no GPU) -> (pixels (n, H, W) uint16,
    bits, status); `out`: an (n, H, W) uint16 array to decode into (planes that are not TIFF_OK keep what it holds)"""
    if out is None:
        out = np.zeros((len(planes), int(H), int(W)), np.uint16)
    assert out.dtype == np.uint16 and out.flags.c_contiguous and out.shape == (len(planes), int(H), int(W))
    bits, status = _tiff_call(lib().tmat_host_tiff_decode_batch, files, planes, H, W, ptr(out), "tmat_host_tiff_decode_batch")
    return out, bits, status


def _stage_pictures_arg(a):
    a = np.asarray(a)
    shape = a.shape
    if a.ndim < 2 or a.size == 0:
        raise ValueError("stage_pictures: expected a non-empty (h, w) image or (n, h, w) batch")
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype not in PIC_DTYPES:
        raise ValueError(f"stage_pictures: dtype {a.dtype} is not one of uint16, float32, float64, uint8")
    a = np.ascontiguousarray(a)
    return (a[None] if a.ndim == 2 else a), shape


def host_stage_pictures(a):
    """tmat_host_stage_pictures: the host twin of Handle.stage_pictures (same bytes, no GPU)"""
    a, shape = _stage_pictures_arg(a)
    out = np.empty(a.shape, np.uint8)
    check(lib().tmat_host_stage_pictures(ptr(a), PIC_DTYPES[a.dtype], a.shape[0], a[0].size, ptr(out)), "tmat_host_stage_pictures")
    return out.reshape(shape)


def host_render_barcode(bars, vis_width=2000):
    """tmat_host_render_barcode: (S, S, 3) u8 with S = round(0.9 vis_width)"""
    bars = np.ascontiguousarray(bars, np.float64).reshape(-1, 2)
    S = int(round(vis_width * 0.9))
    out = np.empty((S, S, 3), np.uint8)
    check(lib().tmat_host_render_barcode(ptr(bars), len(bars), int(vis_width), ptr(out)), "tmat_host_render_barcode")
    return out


def _barcode_args(bars_list):
    """[(k, 2) bars] -> (concatenated (sum k + 1, 2) f64 with one spare row, offsets (n + 1) i32)"""
    arrs = [np.asarray(b, np.float64).reshape(-1, 2) for b in bars_list]
    off = np.zeros(len(arrs) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return np.ascontiguousarray(np.concatenate(arrs + [np.zeros((1, 2))])), off


def host_barcode_rects(bars, vis_width=2000):
    """tmat_host_barcode_rects: the (k, 5) int32 rectangle table (xa, xb, ya, yb, rgb) both barcode rasterisers fill; rows [ya, yb) count
    from the bottom of the canvas, rgb = r | g << 8 | b << 16; empty when nothing is drawn"""
    bars = np.ascontiguousarray(bars, np.float64).reshape(-1, 2)
    out = np.zeros((max(len(bars), 1), 5), np.int32)
    n = C.c_int(0)
    check(lib().tmat_host_barcode_rects(ptr(bars), len(bars), int(vis_width), ptr(out), len(out), C.byref(n)), "tmat_host_barcode_rects")
    return out[: n.value].copy()


# -- host pixel stages (csrc/postproc.cpp); exposed for stage-wise parity tests --------------------
def roi_plan(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), max_classes=16, _export="tmat_roi_plan"):
    """tmat_roi_plan (include/tmat.h): the region plan of the UNet up path for an (hh, ww) image; host arithmetic, no GPU.
    The NESTED rectangles (TMAT_ROI_TIGHT=0); roi_plan_exact returns the ones launched by default.
    Returns a dict: tiles_per_img, n_classes (0: fall-back "everything"), tile_class / tile_rank [tiles_per_img], class_count [max_classes],
    rects [3 n_up + 1][max_classes][4] (y0, x0, rows, columns), mac_planned / mac_full [3 n_up + 1]."""
    L = lib()
    fn = getattr(L, _export)
    fn.argtypes = [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 2 + [C.c_void_p] * 8
    n_up = len(channels) - 1
    aug = (patch + 1) // 2
    cap = 8 * ((hh + 2 * aug - patch) // (patch // 2) + 1) * ((ww + 2 * aug - patch) // (patch // 2) + 1)
    ch = np.asarray(channels, np.int32)
    tpi, ncls = np.zeros(1, np.int32), np.zeros(1, np.int32)
    tcls, trank = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ccount = np.zeros(max_classes, np.int32)
    rects = np.zeros((3 * n_up + 1, max_classes, 4), np.int32)
    mp, mf = np.zeros(3 * n_up + 1), np.zeros(3 * n_up + 1)
    check(fn(hh, ww, patch, n_up, ptr(ch), max_classes, cap, ptr(tpi), ptr(ncls), ptr(tcls), ptr(trank), ptr(ccount),
             ptr(rects), ptr(mp), ptr(mf)), _export[5:])
    n = int(tpi[0])
    return dict(tiles_per_img=n, n_classes=int(ncls[0]), tile_class=tcls[:n], tile_rank=trank[:n], class_count=ccount, rects=rects,
                mac_planned=mp, mac_full=mf)


def roi_plan_tight(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), max_classes=16):
    """tmat_roi_plan_tight (include/tmat.h): roi_plan's classes and patch order with the TIGHT rectangles -- every layer's own need, its
    columns rounded once (what TMAT_ROI_EXACT=0 launches; roi_plan_exact returns the default).  Same dict as roi_plan."""
    return roi_plan(hh, ww, patch, channels, max_classes, _export="tmat_roi_plan_tight")


def roi_plan_exact(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), max_classes=16):
    """tmat_roi_plan_exact (include/tmat.h): roi_plan's classes and patch order with the EXACT rectangles -- every layer's own need, rows
    and columns unrounded -- that the tiled entry points launch by default (TMAT_ROI_EXACT=0: the tight ones).  Same dict as roi_plan."""
    return roi_plan(hh, ww, patch, channels, max_classes, _export="tmat_roi_plan_exact")


def roi_plan_down(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3, max_classes=16):
    """tmat_roi_plan_down (include/tmat.h): the down-path tables of roi_plan's classes; host arithmetic, no GPU.
    Returns a dict: n_classes, rects / needs [6 n_down + 4][max_classes][4] (y0, x0, rows, columns), mac_planned / mac_full /
    bytes_planned / bytes_full [6 n_down + 4], free_tile [n_down]."""
    L = lib()
    L.tmat_roi_plan_down.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 8
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    ncls = np.zeros(1, np.int32)
    rects, needs = np.zeros((nl, max_classes, 4), np.int32), np.zeros((nl, max_classes, 4), np.int32)
    mp, mf, bp, bf = np.zeros(nl), np.zeros(nl), np.zeros(nl), np.zeros(nl)
    free = np.zeros(n_down, np.int32)
    check(L.tmat_roi_plan_down(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), max_classes, ptr(ncls), ptr(rects), ptr(needs),
                               ptr(mp), ptr(mf), ptr(bp), ptr(bf), ptr(free)), "roi_plan_down")
    return dict(n_classes=int(ncls[0]), rects=rects, needs=needs, mac_planned=mp, mac_full=mf, bytes_planned=bp, bytes_full=bf, free_tile=free)


def roi_plan_const(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3, max_classes=16):
    """tmat_roi_plan_const (include/tmat.h): the constant-ring tables of roi_plan_down's plan; host arithmetic, no GPU.
    Returns a dict: n_classes, nonconst / live / rect_live [6 n_down + 4][max_classes][4] (y0, x0, rows, columns),
    fill [6 n_down + 4][max_classes][4 strips][4], stored / mac_live / bytes_live [6 n_down + 4]."""
    L = lib()
    L.tmat_roi_plan_const.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 8
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    ncls = np.zeros(1, np.int32)
    nonconst, live, rect_live = (np.zeros((nl, max_classes, 4), np.int32) for _ in range(3))
    fill = np.zeros((nl, max_classes, 4, 4), np.int32)
    stored = np.zeros(nl, np.int32)
    ml, bl = np.zeros(nl), np.zeros(nl)
    check(L.tmat_roi_plan_const(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), max_classes, ptr(ncls), ptr(nonconst),
                                ptr(live), ptr(rect_live), ptr(fill), ptr(stored), ptr(ml), ptr(bl)), "roi_plan_const")
    return dict(n_classes=int(ncls[0]), nonconst=nonconst, live=live, rect_live=rect_live, fill=fill, stored=stored, mac_live=ml, bytes_live=bl)


def roi_sep_tiles_live(hh, ww, layer, k, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3):
    """tmat_roi_sep_tiles_live (include/tmat.h): roi_sep_tiles for the constant-ring form's rectangles (rect_live)."""
    return roi_sep_tiles(hh, ww, layer, k, patch, channels, down_channels, fused_mask, _export="tmat_roi_sep_tiles_live")


def roi_plan_share(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3, max_classes=16):
    """tmat_roi_plan_share (include/tmat.h): the shared-interior tables of roi_plan_down's plan; host arithmetic, no GPU.
    Returns a dict: n_classes, inner [6 n_down + 4][max_classes][4] (y0, x0, rows, columns), share [6 n_down + 4][max_classes][4]
    (row lo, row hi, column lo, column hi), comp [6 n_down + 4][max_classes][2][patch] uint8, fills [n][7] (layer, class, direction,
    y0, x0, rows, columns), neighbours [tiles_per_img][3]."""
    L = lib()
    L.tmat_roi_plan_share.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 4 +
                                      [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    aug = (patch + 1) // 2
    tiles = 8 * ((hh + 2 * aug - patch) // (patch // 2) + 1) * ((ww + 2 * aug - patch) // (patch // 2) + 1)
    ncls, nfill = np.zeros(1, np.int32), np.zeros(1, np.int32)
    inner, share = np.zeros((nl, max_classes, 4), np.int32), np.zeros((nl, max_classes, 4), np.int32)
    comp = np.zeros((nl, max_classes, 2, patch), np.uint8)
    cap = nl * max_classes * 12
    fills = np.zeros((cap, 7), np.int32)
    nbr = np.zeros((tiles, 3), np.int32)
    check(L.tmat_roi_plan_share(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), max_classes, ptr(ncls), ptr(inner), ptr(share),
                                ptr(comp), cap, ptr(nfill), ptr(fills), tiles, ptr(nbr)), "roi_plan_share")
    return dict(n_classes=int(ncls[0]), inner=inner, share=share, comp=comp, fills=fills[:int(nfill[0])], neighbours=nbr)


def roi_plan_share_rect(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3, max_classes=16):
    """tmat_roi_plan_share_rect (include/tmat.h): the rectangle launches' shared-interior tables of roi_plan_down's plan; host arithmetic,
    no GPU.  Returns a dict: n_classes, share [6 n_down + 4][max_classes][4] (row lo, row hi, column lo, column hi), n_rects
    [6 n_down + 4][max_classes], rects [6 n_down + 4][max_classes][4][4] (y0, x0, rows, columns), comp [6 n_down + 4][max_classes][2][patch]
    uint8, fills [n][7] (layer, class, direction, y0, x0, rows, columns), mac_rect and bytes_rect [6 n_down + 4], any, level, max_segs."""
    L = lib()
    L.tmat_roi_plan_share_rect.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 5 +
                                           [C.c_int] + [C.c_void_p] * 5)
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    ncls, nfill, info = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(3, np.int32)
    share, nrect = np.zeros((nl, max_classes, 4), np.int32), np.zeros((nl, max_classes), np.int32)
    rects = np.zeros((nl, max_classes, 4, 4), np.int32)
    comp = np.zeros((nl, max_classes, 2, patch), np.uint8)
    cap = nl * max_classes * 12
    fills = np.zeros((cap, 7), np.int32)
    mac, byt = np.zeros(nl, np.float64), np.zeros(nl, np.float64)
    check(L.tmat_roi_plan_share_rect(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), max_classes, ptr(ncls), ptr(share),
                                     ptr(nrect), ptr(rects), ptr(comp), cap, ptr(nfill), ptr(fills), ptr(mac), ptr(byt), ptr(info)),
          "roi_plan_share_rect")
    return dict(n_classes=int(ncls[0]), share=share, n_rects=nrect, rects=rects, comp=comp, fills=fills[:int(nfill[0])], mac_rect=mac,
                bytes_rect=byt, any=bool(info[0]), level=int(info[1]), max_segs=int(info[2]))


def roi_plan_share_fused_rect(hh, ww, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3, max_classes=16):
    """tmat_roi_plan_share_fused_rect (include/tmat.h): the shared-interior tables of the fused levels' rectangle launches; host
    arithmetic, no GPU.  Returns a dict: n_classes, n_rects [6 n_down + 4][max_classes], rects [6 n_down + 4][max_classes][4][4] (y0, x0,
    rows, columns), comp [6 n_down + 4][max_classes][2][patch] uint8, fills [n][7] (layer, class, direction, y0, x0, rows, columns: the
    halo strips), fill_on [6 n_down + 4], mac / bytes / px / px_live / copy_old / copy_new [6 n_down + 4], any, levels, max_segs."""
    L = lib()
    L.tmat_roi_plan_share_fused_rect.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 4 +
                                                 [C.c_int] + [C.c_void_p] * 5)
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    ncls, nfill, info = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(3, np.int32)
    nrect = np.zeros((nl, max_classes), np.int32)
    rects = np.zeros((nl, max_classes, 4, 4), np.int32)
    comp = np.zeros((nl, max_classes, 2, patch), np.uint8)
    cap = nl * max_classes * 12
    fills = np.zeros((cap, 7), np.int32)
    on = np.zeros(nl, np.int32)
    tot = np.zeros((nl, 6), np.float64)
    check(L.tmat_roi_plan_share_fused_rect(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), max_classes, ptr(ncls), ptr(nrect),
                                           ptr(rects), ptr(comp), cap, ptr(nfill), ptr(fills), ptr(on), ptr(tot), ptr(info)),
          "roi_plan_share_fused_rect")
    return dict(n_classes=int(ncls[0]), n_rects=nrect, rects=rects, comp=comp, fills=fills[:int(nfill[0])], fill_on=on, mac=tot[:, 0],
                bytes=tot[:, 1], px=tot[:, 2], px_live=tot[:, 3], copy_old=tot[:, 4], copy_new=tot[:, 5], any=bool(info[0]),
                levels=int(info[1]), max_segs=int(info[2]))


ROI_DOWN_FORMS = ("full", "region", "const", "share", "share_rect", "share_fused_rect")      # csrc/roi_plan.h:RoiDownForm, by value


def roi_down_schedule(hh, ww, form, k, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3):
    """tmat_roi_down_schedule (include/tmat.h): what a down pass of k images launches under `form` (a name of ROI_DOWN_FORMS or its value,
    "region" upwards); host arithmetic, no GPU.  Returns a dict: form (the one that runs, by value), stem_layer, max_segs, seg_total,
    segs: per layer of the down plan an array [n][6] (first patch, patches, y0, x0, rows, columns) in launch order, const_fills [n][7]
    (layer, first patch, patches, y0, x0, rows, columns), copies [n][8] (layer, first patch, patches, direction, y0, x0, rows, columns)."""
    L = lib()
    L.tmat_roi_down_schedule.argtypes = ([C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_int, C.c_int] + [C.c_void_p] * 3 +
                                         [C.c_int, C.c_void_p, C.c_void_p] * 2)
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nl = 6 * n_down + 4
    info, nseg, ncf, ncp = np.zeros(4, np.int32), np.zeros(nl, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    segs = np.zeros((nl, 64, 6), np.int32)
    cap = nl * 16 * 12
    cfill, copies = np.zeros((cap, 7), np.int32), np.zeros((cap, 8), np.int32)
    f = ROI_DOWN_FORMS.index(form) if isinstance(form, str) else int(form)
    check(L.tmat_roi_down_schedule(hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), f, int(k), ptr(info), ptr(nseg), ptr(segs),
                                   cap, ptr(ncf), ptr(cfill), cap, ptr(ncp), ptr(copies)), "roi_down_schedule")
    return dict(form=int(info[0]), stem_layer=int(info[1]), max_segs=int(info[2]), seg_total=int(info[3]),
                segs=[segs[l, :int(nseg[l])].copy() for l in range(nl)], const_fills=cfill[:int(ncf[0])], copies=copies[:int(ncp[0])])


def roi_sep_tiles_share(hh, ww, layer, k, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3):
    """tmat_roi_sep_tiles_share (include/tmat.h): roi_sep_tiles for the shared-interior form (the tiles that hold a comp pixel)."""
    return roi_sep_tiles(hh, ww, layer, k, patch, channels, down_channels, fused_mask, _export="tmat_roi_sep_tiles_share")


def roi_sep_quads(hh, ww, layer, k, form="share", patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3):
    """tmat_roi_sep_quads (include/tmat.h): the quadrant table of plain fused layer `layer` (6 b + 1) for a pass of k images under `form`
    (a name of ROI_DOWN_FORMS or its value; "share" upwards); host arithmetic, no GPU.  Returns (ids int32 [4 x packed tiles]: the own
    patches' quadrants, the constant patches', the padding; own: the ids of the pass's own patches; n_ids: all ids before the padding;
    full: the full-frame tile count of the pass's own patches)."""
    L = lib()
    L.tmat_roi_sep_quads.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint] + [C.c_int] * 4 + [C.c_void_p] * 2
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    f = ROI_DOWN_FORMS.index(form) if isinstance(form, str) else int(form)
    counts = np.zeros(4, np.int32)
    args = (hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), f, int(layer), int(k))
    check(L.tmat_roi_sep_quads(*args, 0, ptr(counts), None), "roi_sep_quads")
    ids = np.zeros(max(int(counts[0]), 1), np.int32)
    check(L.tmat_roi_sep_quads(*args, len(ids), ptr(counts), ptr(ids)), "roi_sep_quads")
    return ids[:int(counts[0])], int(counts[1]), int(counts[2]), int(counts[3])


def roi_sep_quads_pool(hh, ww, layer, k, form="share", patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3):
    """tmat_roi_sep_quads_pool (include/tmat.h): roi_sep_quads for the pooled fused layer `layer` (6 b + 3); the same return values."""
    L = lib()
    L.tmat_roi_sep_quads_pool.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint] + [C.c_int] * 4 + [C.c_void_p] * 2
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    f = ROI_DOWN_FORMS.index(form) if isinstance(form, str) else int(form)
    counts = np.zeros(4, np.int32)
    args = (hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), f, int(layer), int(k))
    check(L.tmat_roi_sep_quads_pool(*args, 0, ptr(counts), None), "roi_sep_quads_pool")
    ids = np.zeros(max(int(counts[0]), 1), np.int32)
    check(L.tmat_roi_sep_quads_pool(*args, len(ids), ptr(counts), ptr(ids)), "roi_sep_quads_pool")
    return ids[:int(counts[0])], int(counts[1]), int(counts[2]), int(counts[3])


def debug_share_fill_check(n_patches, side, channels, neighbours, items):
    """tmat_debug_share_fill_check (include/tmat.h): None when the share-fill launcher would take the table, its refusal otherwise.
    Host-side checks only, nothing is launched."""
    L = lib()
    L.tmat_debug_share_fill_check.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p]
    nb = np.ascontiguousarray(neighbours, np.int32).reshape(-1, 3)
    it = np.ascontiguousarray(items, np.int32).reshape(-1, 7)
    rc = L.tmat_debug_share_fill_check(int(n_patches), int(side), int(channels), ptr(nb), len(it), ptr(it))
    return None if rc == 0 else L.tmat_last_error().decode()


def roi_sep_tiles(hh, ww, layer, k, patch=320, channels=(512, 512, 256, 128, 64), down_channels=(64, 128, 256, 512), fused_mask=3,
                  _export="tmat_roi_sep_tiles"):
    """tmat_roi_sep_tiles (include/tmat.h): the full-frame ids of the tiles fused separable layer `layer` visits in a pass of k images;
    host arithmetic, no GPU.  Returns (ids int32 [planned], full-frame tile count)."""
    L = lib()
    fn = getattr(L, _export)
    fn.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_uint] + [C.c_int] * 3 + [C.c_void_p] * 3
    n_up, n_down = len(channels) - 1, len(down_channels) - 1
    ch, dch = np.asarray(channels, np.int32), np.asarray(down_channels, np.int32)
    nt, nf = np.zeros(1, np.int32), np.zeros(1, np.int32)
    args = (hh, ww, patch, n_up, ptr(ch), n_down, ptr(dch), int(fused_mask), int(layer), int(k))
    check(fn(*args, 0, ptr(nt), ptr(nf), None), _export[5:])
    ids = np.zeros(max(int(nt[0]), 1), np.int32)
    check(fn(*args, len(ids), ptr(nt), ptr(nf), ptr(ids)), _export[5:])
    return ids[:int(nt[0])], int(nf[0])


def host_lanczos4_u16(img, out_hw):
    img = np.ascontiguousarray(img, np.uint16)
    out = np.empty(out_hw, np.uint16)
    L = lib()
    L.tmat_host_lanczos4_u16.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    check(L.tmat_host_lanczos4_u16(ptr(img), img.shape[0], img.shape[1], out_hw[0], out_hw[1], ptr(out)), "lanczos4")
    return out


def host_rescale01_u16(img):
    img = np.ascontiguousarray(img, np.uint16)
    out = np.empty(img.shape, np.float32)
    L = lib()
    L.tmat_host_rescale01_u16.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    check(L.tmat_host_rescale01_u16(ptr(img), img.size, ptr(out)), "rescale01")
    return out


def host_rescale255_f32(img):
    img = np.ascontiguousarray(img, np.float32)
    out = np.empty(img.shape, np.float32)
    L = lib()
    L.tmat_host_rescale255_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    check(L.tmat_host_rescale255_f32(ptr(img), img.size, ptr(out)), "rescale255")
    return out


def host_filter_mask(mask, use_median=True, remove_isolated=True):
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    out = np.empty(m.shape, np.uint8)
    L = lib()
    L.tmat_host_filter_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    check(L.tmat_host_filter_mask(ptr(m), m.shape[0], m.shape[1], int(use_median), int(remove_isolated), ptr(out)), "filter")
    return out.astype(bool)


def host_skeletonize(mask):
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    out = np.empty(m.shape, np.uint8)
    L = lib()
    L.tmat_host_skeletonize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    check(L.tmat_host_skeletonize(ptr(m), m.shape[0], m.shape[1], ptr(out)), "skeletonize")
    return out.astype(bool)


def host_medial_axis(mask):
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    sk = np.empty(m.shape, np.uint8)
    dist = np.empty(m.shape, np.float64)
    L = lib()
    L.tmat_host_medial_axis.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    check(L.tmat_host_medial_axis(ptr(m), m.shape[0], m.shape[1], ptr(sk), ptr(dist)), "medial_axis")
    return sk.astype(bool), dist


def host_permutation(seed, n):
    out = np.empty(n, np.uint32)
    L = lib()
    L.tmat_host_permutation.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    check(L.tmat_host_permutation(seed, n, ptr(out)), "permutation")
    return out


def host_postprocess(pred, out_shape):
    pred = np.ascontiguousarray(pred, np.float64)
    out = np.empty(out_shape, np.float32)
    L = lib()
    L.tmat_host_postprocess.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    check(L.tmat_host_postprocess(ptr(pred), pred.shape[0], pred.shape[1], out_shape[0], out_shape[1], ptr(out)), "postprocess")
    return out
