"""ctypes binding of libvs_amd.so (the C ABI declared in include/vs_amd.h).

This is plumbing for the Python tests and bench.py: every compute call goes through the C ABI
into the hand-written gfx950 kernels.  There is no fallback -- a missing library raises.

numpy arrays are passed as VS_MEM_HOST; for VS_MEM_DEVICE pass raw device pointers (ints), e.g.
torch tensors' data_ptr().

The file is ordered by pass: a pass's params constructor, host form and device form lie together.  In front of the passes
lie the structs and the SIGNATURES table, then the helpers every wrapper marshals its arguments with -- each decision is
made in one of them, once.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VS_AMD_LIB", os.path.join(_HERE, "libvs_amd.so"))

MEM_HOST, MEM_DEVICE = 0, 1
FMT_GRAY8, FMT_BGR8 = 0, 1
FMT_BGR10, FMT_BGR12, FMT_BGR16_FULL = 2, 3, 4      # u16 containers: bits the samples use
WARP_LANCZOS2, WARP_BILINEAR, WARP_LANCZOS2_FAST, WARP_LANCZOS2_SEP, WARP_BILINEAR_CV = 0, 1, 2, 3, 4
BORDER_CLAMP, BORDER_CONSTANT = 0, 1
RESIZE_LINEAR, RESIZE_AREA = 0, 1
SELECT_STL_HOST, SELECT_DEVICE, SELECT_STABLE = 0, 1, 2
BATCH_EXCLUSIVE, BATCH_SHARED = 0, 1
ABI_VERSION = 5                                     # VS_ABI_VERSION of include/vs_amd.h


class Transform(C.Structure):
    _fields_ = [("A", C.c_double), ("B", C.c_double), ("TX", C.c_double), ("TY", C.c_double)]

    def tup(self):
        return (self.A, self.B, self.TX, self.TY)

    @staticmethod
    def of(A=0.0, B=0.0, TX=0.0, TY=0.0):
        return Transform(float(A), float(B), float(TX), float(TY))


class Point(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double)]


class AlignerParams(C.Structure):
    _fields_ = [("phase_correlate", C.c_int), ("phase_correlate_threshold", C.c_double),
                ("threshold", C.c_double), ("smallest_fraction", C.c_float), ("max_iters", C.c_int),
                ("pyramid_min_width", C.c_int), ("pyramid_min_height", C.c_int),
                ("max_displacement", C.c_double)]


class StabilizerParams(C.Structure):
    _fields_ = [("aligner", AlignerParams), ("lag", C.c_int), ("smoother_memory", C.c_int),
                ("lambda_", C.c_double), ("enable_smoother", C.c_int), ("crop_pixels", C.c_int),
                ("min_disp", C.c_double), ("max_disp", C.c_double), ("min_decay", C.c_double),
                ("max_decay", C.c_double), ("warp_mode", C.c_int), ("warp_border", C.c_int)]


class AlignInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("fail_reason", C.c_int32), ("fail_level", C.c_int32),
                ("levels", C.c_int32), ("iterations", C.c_int32 * 16), ("condition", C.c_double * 16),
                ("phase_dx", C.c_double), ("phase_dy", C.c_double), ("phase_response", C.c_double),
                ("selected_x", C.c_int32 * 16), ("selected_y", C.c_int32 * 16), ("level_transform", Transform * 16)]


STAGES = ["ingest", "pyr_down", "keyframe", "warpdiff", "select", "gather", "gn", "phase"]


class StageTimings(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_int64 * 8), ("frames", C.c_int64), ("gn_iterations", C.c_int64)]


class FlowParams(C.Structure):
    """vs_flow_params: cv::calcOpticalFlowFarneback's parameters (levels = layers above the frame)"""
    _fields_ = [("pyr_scale", C.c_double), ("levels", C.c_int), ("winsize", C.c_int), ("iterations", C.c_int),
                ("poly_n", C.c_int), ("poly_sigma", C.c_double), ("flags", C.c_int)]

    def tup(self):
        return (self.pyr_scale, self.levels, self.winsize, self.iterations, self.poly_n, self.poly_sigma, self.flags)


class DeblurParams(C.Structure):
    """vs_deblur_params: sensitivity in gray levels, max_ratio bounds a candidate's sharpness ratio"""
    _fields_ = [("sensitivity", C.c_float), ("max_ratio", C.c_float)]


class DenoiseParams(C.Structure):
    """vs_denoise_params: strength in 8-bit levels, 1 .. 255"""
    _fields_ = [("strength", C.c_int)]


class RollingParams(C.Structure):
    """vs_rolling_params: readout, the share of the frame period the sensor takes from row 0 to row h - 1, -1 .. 1"""
    _fields_ = [("readout", C.c_double)]


class LensParams(C.Structure):
    """vs_lens_params: the radial lens model (OpenCV's distCoeffs order k1, k2, p1, p2, k3, k4, k5, k6), the output camera's zoom and the border
    the stabilizer's correction remaps with"""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "zoom")] + [("border", C.c_int)]

    def tup(self):
        return tuple(getattr(self, k) for k, _ in self._fields_)


class DeflickerParams(C.Structure):
    """vs_deflicker_params: the lattice step of the exposure statistics, 1 .. 64"""
    _fields_ = [("step", C.c_int)]


class SceneParams(C.Structure):
    """vs_scene_params: the lattice step of the scene-cut statistics, 1 .. 64; the threshold in 8-bit levels, 1 .. 255"""
    _fields_ = [("step", C.c_int), ("threshold", C.c_int)]


class FidelityScore(C.Structure):
    """vs_fidelity_score: PSNR per channel, pooled and on gray, in dB (inf for identical images); the mean SSIM (NaN without a window)"""
    _fields_ = [(k, C.c_double) for k in ("psnr_b", "psnr_g", "psnr_r", "psnr", "psnr_y", "ssim")]

    def tup(self):
        return tuple(getattr(self, k) for k, _ in self._fields_)


class SharpenParams(C.Structure):
    """vs_sharpen_params: the strength in sixteenths of the two-tap filter's own variance, 1 .. 32"""
    _fields_ = [("strength", C.c_int)]


class FillBlendParams(C.Structure):
    """vs_fill_blend_params: feather 0 (off) or 1 .. 6; match 0 or 1"""
    _fields_ = [("feather", C.c_int), ("match", C.c_int)]


class VsError(RuntimeError):
    pass


_vp, _i32, _f32, _f64, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t


class YcbcrPlanes(C.Structure):
    """vs_ycbcr_planes: frame 0's first samples, strides in elements; cb == cr == None: luma only"""
    _fields_ = [("y", _vp), ("cb", _vp), ("cr", _vp), ("y_stride", _i32), ("c_stride", _i32), ("c_step", _i32), ("sub_x", _i32), ("sub_y", _i32),
                ("y_frame_stride", _sz), ("c_frame_stride", _sz)]


# the pointer types the table repeats: int*, int32_t*, int64_t*, double*, and a pointer to each struct of the header
_IP, _I32P, _I64P, _F64P = C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
_TP, _YP = C.POINTER(Transform), C.POINTER(YcbcrPlanes)
_AlignerP, _StabilizerP, _FlowP = C.POINTER(AlignerParams), C.POINTER(StabilizerParams), C.POINTER(FlowParams)
_FillBlendP, _DeblurP, _DenoiseP, _RollingP = C.POINTER(FillBlendParams), C.POINTER(DeblurParams), C.POINTER(DenoiseParams), C.POINTER(RollingParams)
_LensP, _DeflickerP, _SceneP, _SharpenP = C.POINTER(LensParams), C.POINTER(DeflickerParams), C.POINTER(SceneParams), C.POINTER(SharpenParams)

# name -> (restype, argtypes).  tests/test_capi_symbols.py holds every row of this table against the prototype of the same
# name in include/vs_amd.h: the return type, the argument count and every argument's kind.
SIGNATURES = {
    "vs_last_error": (C.c_char_p, []),
    "vs_version": (C.c_char_p, []),
    "vs_abi_version": (_i32, []),
    "vs_sizeof_align_info": (_sz, []),
    "vs_test_fail_alloc": (_i32, [_i32]),
    "vs_debug_bounds_check": (_i32, []),
    "vs_debug_bounds_selftest": (_i32, []),
    "vs_device_count": (_i32, []),
    "vs_shader_clock_probe": (_i32, [_vp, _F64P]),
    "vs_stream_retire": (_i32, [_vp]),
    "vs_format_bits": (_i32, [_i32]),
    "vs_format_max_value": (_i32, [_i32]),
    "vs_aligner_stream": (_vp, [_vp]),
    "vs_aligner_wait_stream": (_i32, [_vp, _vp]),
    "vs_stabilizer_stream": (_vp, [_vp]),
    "vs_stabilizer_wait_stream": (_i32, [_vp, _vp]),
    "vs_aligner_params_default": (None, [_AlignerP]),
    "vs_stabilizer_params_default": (None, [_StabilizerP]),
    "vs_transform_inverse": (Transform, [_TP]),
    "vs_transform_compose": (Transform, [_TP, _TP]),
    "vs_transform_warp": (Point, [_TP, Point]),
    "vs_transform_warp_center": (Point, [_TP, Point, _f64, _f64]),
    "vs_transform_max_corner_displacement": (_f64, [_TP, _f64, _f64]),
    "vs_tile_size": (_i32, [_i32, _i32]),
    "vs_ul_params_sparse": (None, [_TP, _i32, _i32, _vp]),
    "vs_ul_params_warp": (None, [_TP, _i32, _i32, _vp]),
    "vs_cv_inverse_matrix": (None, [_TP, _i32, _i32, _vp]),
    "vs_smoother_create": (_vp, [_i32, _i32, _f64]),
    "vs_smoother_destroy": (None, [_vp]),
    "vs_smoother_update": (_i32, [_vp, _TP, _TP]),
    "vs_tvl1_smooth": (None, [_vp, _i32, _f64, _i32, _vp]),
    "vs_calib_copy12": (_i32, [_vp, _vp, _sz, _vp]),
    "vs_pyr_down": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "vs_grad_xy": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vs_grad_argmax": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vs_sparse_jac": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vs_keyframe_fused": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "vs_sparse_warpdiff": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _f32, _f32, _f32, _f32, _vp, _i32, _vp]),
    "vs_sparse_ica": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _f32, _f32, _f32, _f32, _vp, _i32, _vp]),
    "vs_select_smallest": (_i32, [_vp, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "vs_select_smallest_stable": (_i32, [_vp, _i32, _i32, _i32, _f32, _vp, _i32, _vp]),
    "vs_phase_correlate": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vs_optimal_dft_size": (_i32, [_i32]),
    "vs_image_warp": (_i32, [_vp, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _vp, _i32, _i32, _i32, _vp]),
    "vs_bgr_image_warp": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _TP, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "vs_bgr_image_warp_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _TP, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_image_warp_roi_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _TP, _i32, _i32, _i32,
                                           _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_image_warp_fill_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _i32, _i32,
                                            _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_channel_sums_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "vs_bgr_image_warp_fill_blend_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _vp,
                                                  _FillBlendP, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_deblur_params_default": (None, [_DeblurP]),
    "vs_bgr_sharpness_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "vs_bgr_deblur_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _I32P, _TP, _DeblurP,
                                   _vp, _sz, _i32, _i32, _vp]),
    "vs_denoise_params_default": (None, [_DenoiseP]),
    "vs_bgr_denoise_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _DenoiseP,
                                    _vp, _sz, _i32, _i32, _vp]),
    "vs_rolling_params_default": (None, [_RollingP]),
    "vs_bgr_rolling_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _RollingP,
                                    _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_remap_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_resize_taps": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp]),
    "vs_bgr_resize_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _i32, _i32, _vp]),
    "vs_ycbcr_to_bgr_batch": (_i32, [_YP, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_to_ycbcr_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _YP, _i32, _vp]),
    "vs_stabilizer_process_batch_ycbcr": (_i32, [_vp, _YP, _i32, _i32, _i32, _i32, _i32, _YP, _I32P, _IP, _IP]),
    "vs_lens_params_default": (None, [_LensP, _i32, _i32]),
    "vs_lens_map": (_i32, [_LensP, _i32, _i32, _vp, _i32, _i32, _vp]),
    "vs_deflicker_params_default": (None, [_DeflickerP]),
    "vs_bgr_exposure_stats_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _DeflickerP,
                                           _vp, _i32, _vp]),
    "vs_exposure_gains_batch": (_i32, [_vp, _i32, _i32, _i32, _i32, _DeflickerP, _vp, _i32, _vp]),
    "vs_bgr_gain_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _i32, _i32, _vp]),
    "vs_scene_params_default": (None, [_SceneP]),
    "vs_bgr_scene_stats_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _TP, _SceneP, _vp, _i32, _vp]),
    "vs_scene_cuts": (_i32, [_vp, _i32, _i32, _i32, _SceneP, _vp]),
    "vs_bgr_fidelity_batch": (_i32, [_vp, _sz, _i32, _i32, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _I32P, _vp, _i32, _vp]),
    "vs_fidelity_scores": (_i32, [_vp, _i32, _i32, _i32, _i32, C.POINTER(FidelityScore)]),
    "vs_bgr_fill_coverage_batch": (_i32, [_i32, _i32, _i32, _i32, _I32P, _TP, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_sharpen_params_default": (None, [_SharpenP]),
    "vs_bgr_sharpen_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _TP, _SharpenP, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_inpaint_batch": (_i32, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _i32, _i32, _vp]),
    "vs_bgr_image_warp_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _TP, _i32, _i32, _vp, _i32, _i32, _vp]),
    "vs_bgr_to_gray": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "vs_flow_params_default": (None, [_FlowP]),
    "vs_flow_create": (_vp, [_FlowP, _i32]),
    "vs_flow_destroy": (None, [_vp]),
    "vs_flow_compute": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32]),
    "vs_flow_jitter": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _F64P]),
    "vs_aligner_create": (_vp, [_AlignerP, _i32]),
    "vs_aligner_destroy": (None, [_vp]),
    "vs_aligner_set_select_mode": (_i32, [_vp, _i32]),
    "vs_stabilizer_set_select_mode": (_i32, [_vp, _i32]),
    "vs_aligner_get_select_mode": (_i32, [_vp]),
    "vs_stabilizer_get_select_mode": (_i32, [_vp]),
    "vs_stabilizer_set_border_fill": (_i32, [_vp, _i32]),
    "vs_stabilizer_get_border_fill": (_i32, [_vp]),
    "vs_stabilizer_set_fill_blend": (_i32, [_vp, _FillBlendP]),
    "vs_stabilizer_get_fill_blend": (_i32, [_vp, _FillBlendP]),
    "vs_stabilizer_set_deblur": (_i32, [_vp, _i32, _DeblurP]),
    "vs_stabilizer_get_deblur": (_i32, [_vp]),
    "vs_stabilizer_set_denoise": (_i32, [_vp, _i32, _DenoiseP]),
    "vs_stabilizer_get_denoise": (_i32, [_vp]),
    "vs_stabilizer_set_rolling_shutter": (_i32, [_vp, _RollingP]),
    "vs_stabilizer_get_rolling_shutter": (_i32, [_vp, _RollingP]),
    "vs_stabilizer_set_lens": (_i32, [_vp, _LensP, _i32, _i32]),
    "vs_stabilizer_get_lens": (_i32, [_vp, _LensP, _IP, _IP]),
    "vs_stabilizer_set_deflicker": (_i32, [_vp, _i32, _DeflickerP]),
    "vs_stabilizer_get_deflicker": (_i32, [_vp]),
    "vs_stabilizer_set_scene_cut": (_i32, [_vp, _SceneP]),
    "vs_stabilizer_get_scene_cut": (_i32, [_vp, _SceneP]),
    "vs_stabilizer_get_scene_cuts": (_i32, [_vp, _I64P, _i32]),
    "vs_stabilizer_set_sharpen": (_i32, [_vp, _SharpenP]),
    "vs_stabilizer_get_sharpen": (_i32, [_vp, _SharpenP]),
    "vs_stabilizer_set_output_size": (_i32, [_vp, _i32, _i32, _i32]),
    "vs_stabilizer_get_output_size": (_i32, [_vp, _IP, _IP, _IP]),
    "vs_stabilizer_set_inpaint": (_i32, [_vp, _i32]),
    "vs_stabilizer_get_inpaint": (_i32, [_vp]),
    "vs_aligner_set_batch_mode": (_i32, [_vp, _i32]),
    "vs_aligner_reset": (_i32, [_vp]),
    "vs_aligner_align_next": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _AlignerP, _TP]),
    "vs_aligner_align_batch": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _AlignerP, _TP, _I32P]),
    "vs_aligner_align_clips": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _AlignerP, _TP, _I32P]),
    "vs_aligner_enable_timing": (_i32, [_vp, _i32]),
    "vs_aligner_get_timings": (_i32, [_vp, C.POINTER(StageTimings)]),
    "vs_aligner_get_info": (_i32, [_vp, _i32, C.POINTER(AlignInfo)]),
    "vs_aligner_level_dims": (_i32, [_vp, _i32, _IP, _IP, _IP, _IP, _IP]),
    "vs_aligner_read_level_image": (_i32, [_vp, _i32, _i32, _vp]),
    "vs_aligner_read_level_argmax": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "vs_aligner_read_level_jacobian": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "vs_stabilizer_create": (_vp, [_StabilizerP, _i32]),
    "vs_stabilizer_destroy": (None, [_vp]),
    "vs_stabilizer_process": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _IP, _IP]),
    "vs_stabilizer_process_batch": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _I32P, _IP, _IP]),
    "vs_stabilizer_process_clips": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _I32P, _IP, _IP]),
    "vs_stabilizer_reset": (_i32, [_vp]),
    "vs_stabilizer_state": (None, [_vp, _TP, _TP, _IP]),
}

_lib = None


def lib():
    """Load libvs_amd.so.  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VsError("libvs_amd.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    # VS_AMD_LIB_PARTIAL=1 (tests/test_host_sanitizers.py): VS_AMD_LIB is a build of the HOST translation unit alone (vs_host.cpp under
    # AddressSanitizer / UBSan, plain g++): only the symbols it has are bound; anything else raises AttributeError where it is used
    partial = os.environ.get("VS_AMD_LIB_PARTIAL") == "1"
    for name, (res, args) in SIGNATURES.items():
        if partial and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.vs_abi_version() != ABI_VERSION or L.vs_sizeof_align_info() != C.sizeof(AlignInfo):
        raise VsError("libvs_amd.so has ABI %d (vs_align_info %d bytes); this binding was written for ABI %d (%d bytes)"
                      % (L.vs_abi_version(), L.vs_sizeof_align_info(), ABI_VERSION, C.sizeof(AlignInfo)))
    _lib = L
    return L


def _check(r):
    if r < 0:
        raise VsError("vs_amd error %d: %s" % (r, lib().vs_last_error().decode()))
    return r


# ---- marshalling: one helper per decision, used by every wrapper below -----------------------
# Foreign-call conversion happens in these four and in _frames_in / _frames_out: a numpy array or a raw address as void*, an optional struct
# by reference, a stream, an int32 array, a Transform array.
def _p(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ref(s):
    """an optional struct by reference: None is the library's own default (or "off")"""
    return C.byref(s) if s is not None else None


def _stream(s):
    """a raw hipStream_t value; None or 0: the default stream"""
    return C.c_void_p(s) if s else None


def _i32p(a):
    return a.ctypes.data_as(_I32P)


def _transforms(ts, n):
    """n Transforms as a ctypes array with at least one element; a ctypes array (what align_* gave with raw=True) is passed through as is, so
    that no per-frame Python objects are made"""
    return ts if isinstance(ts, C.Array) else (Transform * max(n, 1))(*ts)


def _fmt_of(frame_dtype, ndim_tail):
    if ndim_tail == 2:
        return FMT_GRAY8
    return FMT_BGR8 if frame_dtype == np.uint8 else FMT_BGR10      # u16 numpy frames are 10-bit unless the caller passes fmt=


def _channels(fmt):
    return 1 if fmt == FMT_GRAY8 else 3


def _depth(dtype, max_value):
    """(bits of the container, the value the warps saturate at: the container's largest unless the caller says otherwise)"""
    bits = 8 if dtype == np.uint8 else 16
    return bits, ((255 if bits == 8 else 65535) if max_value is None else max_value)


def _pitched(src, stride):
    """(n,h,w,c) -> (n,h,stride) with the rows' own elements in front (the padding is zero)"""
    n, h, w, c = src.shape
    if stride == w * c:
        return src.reshape(n, h, w * c)
    wide = np.zeros((n, h, stride), src.dtype)
    wide[:, :, :w * c] = src.reshape(n, h, w * c)
    return wide


def _frames_in(src, fmt=None, src_stride=None):
    """frames in: src (n,h,w,c) numpy -> the contiguous frames, the format (u16 frames are 10-bit unless fmt says otherwise), the row stride in
    elements (dense unless src_stride says otherwise) and the frames as rows of that stride"""
    src = np.ascontiguousarray(src)
    n, h, w, c = src.shape
    ss = w * c if src_stride is None else src_stride
    return src, (_fmt_of(src.dtype, 3) if fmt is None else fmt), ss, _pitched(src, ss)


def _frames_out(n, h, w, c, dtype, dst_stride=None, guard=None, fill=0):
    """frames out: the padded destination of n frames of h rows of w * c elements -- rows of dst_stride elements (dense unless it says
    otherwise), at least one frame so that there is an address to hand over, every element `guard`, or `fill` without one -- and its row stride"""
    ds = w * c if dst_stride is None else dst_stride
    return np.full((max(n, 1), h, ds), fill if guard is None else guard, dtype), ds


def _cut(out, shape, guard):
    """the frames of `shape` = (n, h, w[, c]) out of their padded destination; with a guard the padded buffer is returned as well, so that the
    caller can see that the padding was left alone"""
    res = np.ascontiguousarray(out[:shape[0], :, :int(np.prod(shape[2:]))]).reshape(shape)
    return (res, out) if guard is not None else res


def _window(roi, w, h):
    return roi if roi is not None else (0, 0, w, h)


def _candidates(cand_frame, cand_t):
    """the candidate lists of the look-ahead passes (fill, deblur, denoise, rolling shutter, exposure statistics, coverage): cand_frame
    (n_out, n_cand) ints, cand_t n_out lists of n_cand Transforms -> the int32 indices, n_out, n_cand, the Transform array.  The library reads
    n_out * n_cand Transforms, so a shorter cand_t is refused here, for host and device forms alike"""
    idx = _c(cand_frame, np.int32)
    n_out, n_cand = idx.shape if idx.ndim == 2 else (0, 0)
    flat = [t for row in cand_t for t in row]
    assert len(flat) == n_out * n_cand
    return idx, n_out, n_cand, _transforms(flat, len(flat))


def _pairs(pair_frames):
    """pair_frames (n_pairs, 2) ints -> the int32 indices, n_pairs"""
    idx = _c(pair_frames, np.int32).reshape(-1, 2)
    return idx, idx.shape[0]


def _params(cls, default, kw, *lead):
    """the constructor behind every *_params(): a `cls` with the library's defaults (`default`, called with the struct and `lead`), fields
    overridden by keyword"""
    p = cls()
    getattr(lib(), default)(C.byref(p), *lead)
    _set_fields(p, kw)
    return p


def _set_fields(p, kw, inner=None):
    """a name that is no field of p is one of `inner`, a struct inside p, or a TypeError: a plain attribute on a ctypes struct would be ignored
    without a word"""
    for k, v in kw.items():
        if k in dict(p._fields_):
            setattr(p, k, v)
        elif inner is not None and k in dict(inner._fields_):
            setattr(inner, k, v)
        else:
            raise TypeError("%s has no field %r" % (type(p).__name__, k))


class _Handle:
    """a handle of the library: made by `_create` (a null handle raises with the library's error text), destroyed with the object"""
    _create = _destroy = None

    def _open(self, *args):
        self.h = getattr(lib(), self._create)(*args)
        if not self.h:
            raise VsError("%s failed: %s" % (self._create, lib().vs_last_error().decode()))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:      # (the module may be half torn down at interpreter exit)
            getattr(_lib, self._destroy)(self.h)
            self.h = None


# ---- the library itself ----------------------------------------------------------------------
def device_count():
    return lib().vs_device_count()


def shader_clock_probe(stream=None):
    """shader clock in MHz as a VALU-bound probe kernel on `stream` sees it (s_memtime / s_memrealtime)"""
    mhz = C.c_double(0.0)
    _check(lib().vs_shader_clock_probe(_stream(stream), C.byref(mhz)))
    return mhz.value


def debug_bounds_check():
    """bounds build only: violations since the last call (0 = clean); raises VsError in the regular library"""
    r = _check(lib().vs_debug_bounds_check())
    return r, (lib().vs_last_error().decode() if r else "")


def test_fail_alloc(k):
    """fault injection: the k-th allocation of the library from now on fails once (0 disarms); returns the allocations seen since the last call"""
    return lib().vs_test_fail_alloc(int(k))


# ---- host-side algebra ---------------------------------------------------------------------
def t_inverse(t):
    return lib().vs_transform_inverse(C.byref(t))


def t_compose(t1, t2):
    return lib().vs_transform_compose(C.byref(t1), C.byref(t2))


def t_warp(t, x, y, center=None):
    if center is None:
        p = lib().vs_transform_warp(C.byref(t), Point(x, y))
    else:
        p = lib().vs_transform_warp_center(C.byref(t), Point(x, y), center[0], center[1])
    return p.x, p.y


def t_max_corner_displacement(t, w, h):
    return lib().vs_transform_max_corner_displacement(C.byref(t), w, h)


def tile_size(w, h):
    return lib().vs_tile_size(w, h)


def ul_params_sparse(t, w, h):
    out = np.empty(4, np.float32)
    lib().vs_ul_params_sparse(C.byref(t), w, h, _p(out))
    return out


def ul_params_warp(t, w, h):
    out = np.empty(4, np.float32)
    lib().vs_ul_params_warp(C.byref(t), w, h, _p(out))
    return out


def cv_inverse_matrix(t, w, h):
    """VS_WARP_BILINEAR_CV's output -> source matrix for the FORWARD transform t (cv::warpAffine's inversion of imgproc.cpp:457-466's matrix)"""
    out = np.empty(6, np.float64)
    lib().vs_cv_inverse_matrix(C.byref(t), w, h, _p(out))
    return out


def tvl1_smooth(data, lam, iterations=100):
    d = _c(data, np.float64)
    out = np.empty_like(d)
    lib().vs_tvl1_smooth(_p(d), d.size, lam, iterations, _p(out))
    return out


class Smoother(_Handle):
    """L1SmootherCenter (smoother.hpp:10-30)"""
    _create, _destroy = "vs_smoother_create", "vs_smoother_destroy"

    def __init__(self, lag_behind, lag_ahead, lam):
        self._open(lag_behind, lag_ahead, lam)

    def update(self, meas):
        out = Transform()
        ok = lib().vs_smoother_update(self.h, C.byref(meas), C.byref(out))
        return bool(ok), out


# ---- kernel level (host-staged numpy convenience wrappers) ---------------------------------
def pyr_down(img):
    img = _c(img, np.uint8)
    h, w = img.shape
    out = np.empty((h // 2, w // 2), np.uint8)
    _check(lib().vs_pyr_down(_p(img), w, h, w, _p(out), w // 2, h // 2, w // 2, MEM_HOST, None))
    return out


def grad_xy(img):
    img = _c(img, np.uint8)
    h, w = img.shape
    gx = np.empty((h, w), np.float32)
    gy = np.empty((h, w), np.float32)
    _check(lib().vs_grad_xy(_p(img), w, h, w, _p(gx), _p(gy), MEM_HOST, None))
    return gx, gy


def grad_argmax(gx, gy, ts=None):
    gx = _c(gx, np.float32)
    gy = _c(gy, np.float32)
    h, w = gx.shape
    if ts is None:
        ts = tile_size(w, h)
    tx, ty = w // ts, h // ts
    lmx = np.empty((2, ty, tx), np.uint16)
    lmy = np.empty((2, ty, tx), np.uint16)
    _check(lib().vs_grad_argmax(_p(gx), _p(gy), w, h, ts, _p(lmx), _p(lmy), MEM_HOST, None))
    return ts, lmx, lmy


def sparse_jac(gx, gy, lmx, lmy):
    gx = _c(gx, np.float32)
    gy = _c(gy, np.float32)
    lmx = _c(lmx, np.uint16)
    lmy = _c(lmy, np.uint16)
    h, w = gx.shape
    _, ty, tx = lmx.shape
    jx = np.empty((4, ty, tx), np.float32)
    jy = np.empty((4, ty, tx), np.float32)
    _check(lib().vs_sparse_jac(_p(gx), _p(gy), w, h, _p(lmx), _p(lmy), tx, ty, _p(jx), _p(jy), MEM_HOST, None))
    return jx, jy


def keyframe_fused(img, ts=None):
    img = _c(img, np.uint8)
    h, w = img.shape
    if ts is None:
        ts = tile_size(w, h)
    tx, ty = w // ts, h // ts
    lmx = np.empty((2, ty, tx), np.uint16)
    lmy = np.empty((2, ty, tx), np.uint16)
    jx = np.empty((4, ty, tx), np.float32)
    jy = np.empty((4, ty, tx), np.float32)
    _check(lib().vs_keyframe_fused(_p(img), w, h, w, ts, _p(lmx), _p(lmy), _p(jx), _p(jy), MEM_HOST, None))
    return ts, lmx, lmy, jx, jy


def sparse_warpdiff_raw(tmpl, key, lm, A, B, TX, TY):
    tmpl = _c(tmpl, np.uint8)
    key = _c(key, np.uint8)
    lm = _c(lm, np.uint16)
    h, w = key.shape
    _, ty, tx = lm.shape
    out = np.empty((ty, tx), np.uint16)
    _check(lib().vs_sparse_warpdiff(_p(tmpl), _p(key), w, h, w, _p(lm), tx, ty, A, B, TX, TY, _p(out), MEM_HOST, None))
    return out


def sparse_warpdiff(tmpl, key, lm, t):
    """SparseWarpDiff (imgproc.cpp:80-106): t is the centre-based transform"""
    h, w = key.shape
    p = ul_params_sparse(t, w, h)
    return sparse_warpdiff_raw(tmpl, key, lm, float(p[0]), float(p[1]), float(p[2]), float(p[3]))


def sparse_ica_raw(tmpl, key, selx, sely, jacx, jacy, A, B, TX, TY):
    tmpl = _c(tmpl, np.uint8)
    key = _c(key, np.uint8)
    selx = _c(selx, np.uint16)
    sely = _c(sely, np.uint16)
    jacx = _c(jacx, np.float32)
    jacy = _c(jacy, np.float32)
    h, w = key.shape
    out = np.empty(4, np.float64)
    _check(lib().vs_sparse_ica(_p(tmpl), _p(key), w, h, w, _p(selx), selx.shape[1], _p(sely), sely.shape[1],
                               _p(jacx), _p(jacy), A, B, TX, TY, _p(out), MEM_HOST, None))
    return out


def sparse_ica(tmpl, key, selx, sely, jacx, jacy, t):
    """SparseICA (imgproc.cpp:46-78)"""
    h, w = key.shape
    p = ul_params_sparse(t, w, h)
    return sparse_ica_raw(tmpl, key, selx, sely, jacx, jacy, float(p[0]), float(p[1]), float(p[2]), float(p[3]))


def select_smallest(warpdiff, fraction=0.8):
    """warpdiff: (ty,tx) or (n,ty,tx) u16.  returns (list of idx arrays, status array)"""
    wd = _c(warpdiff, np.uint16)
    if wd.ndim == 2:
        wd = wd[None]
    n, ty, tx = wd.shape
    idx = np.empty((n, ty * tx), np.int32)
    status = np.empty(n, np.int32)
    cnt = _check(lib().vs_select_smallest(_p(wd), n, tx, ty, fraction, _p(idx), _p(status), MEM_HOST, None))
    return [idx[i, :cnt].copy() for i in range(n)], status


def select_smallest_stable(warpdiff, fraction=0.8):
    """the same step under VS_SELECT_STABLE's rule.  warpdiff: (ty,tx) or (n,ty,tx) u16.  returns a list of idx arrays"""
    wd = _c(warpdiff, np.uint16)
    if wd.ndim == 2:
        wd = wd[None]
    n, ty, tx = wd.shape
    idx = np.empty((n, ty * tx), np.int32)
    cnt = _check(lib().vs_select_smallest_stable(_p(wd), n, tx, ty, fraction, _p(idx), MEM_HOST, None))
    return [idx[i, :cnt].copy() for i in range(n)]


def optimal_dft_size(n):
    return lib().vs_optimal_dft_size(int(n))


def phase_correlate(a, b, want_surface=False):
    """cv::phaseCorrelate on two u8 images -> (dx, dy, response[, unshifted surface (M, N)])"""
    a = _c(a, np.uint8)
    b = _c(b, np.uint8)
    h, w = a.shape
    res = np.zeros(3, np.float64)
    surf = np.empty((optimal_dft_size(h), optimal_dft_size(w)), np.float32) if want_surface else None
    _check(lib().vs_phase_correlate(_p(a), _p(b), w, h, w, MEM_HOST, None, _p(surf) if want_surface else None, _p(res)))
    return (res[0], res[1], res[2], surf) if want_surface else (res[0], res[1], res[2])


def image_warp_raw(img, A, B, TX, TY, out_shape=None):
    img = _c(img, np.uint8)
    h, w = img.shape
    oh, ow = out_shape if out_shape else (h, w)
    out = np.empty((oh, ow), np.float32)
    _check(lib().vs_image_warp(_p(img), w, h, w, A, B, TX, TY, _p(out), ow, oh, MEM_HOST, None))
    return out


def image_warp(img, t):
    """ImageWarp (imgproc.cpp:116-133)"""
    h, w = img.shape
    p = ul_params_warp(t, w, h)
    return image_warp_raw(img, float(p[0]), float(p[1]), float(p[2]), float(p[3]))


def bgr_to_gray(src, shift_to_8=None):
    src = np.ascontiguousarray(src)
    h, w, _ = src.shape
    bits = 8 if src.dtype == np.uint8 else 16
    if shift_to_8 is None:
        shift_to_8 = 0 if bits == 8 else 2
    out = np.empty((h, w), np.uint8)
    _check(lib().vs_bgr_to_gray(_p(src), w, h, w * 3, bits, shift_to_8, _p(out), w, MEM_HOST, None))
    return out


# ---- the warps -------------------------------------------------------------------------------
def bgr_image_warp(src, t, mode=WARP_LANCZOS2, border=BORDER_CLAMP, max_value=None, f32=False):
    src = np.ascontiguousarray(src)
    assert src.dtype in (np.uint8, np.uint16) and src.ndim == 3
    h, w, c = src.shape
    bits, max_value = _depth(src.dtype, max_value)
    if f32:
        out = np.empty((h, w, c), np.float32)
        _check(lib().vs_bgr_image_warp_f32(_p(src), w, h, w * c, c, bits, C.byref(t), mode, border, _p(out), w * c, MEM_HOST, None))
        return out
    out = np.empty_like(src)
    _check(lib().vs_bgr_image_warp(_p(src), w, h, w * c, c, bits, C.byref(t), mode, border, max_value, _p(out), w * c, MEM_HOST, None))
    return out


def bgr_image_warp_batch(src, ts, mode=WARP_LANCZOS2, border=BORDER_CLAMP, max_value=None):
    """src (n,h,w,c) numpy; ts list of Transform"""
    src = np.ascontiguousarray(src)
    n, h, w, c = src.shape
    bits, max_value = _depth(src.dtype, max_value)
    out = np.empty_like(src)
    _check(lib().vs_bgr_image_warp_batch(_p(src), h * w * c, n, w, h, w * c, c, bits, _transforms(ts, n), mode, border, max_value,
                                         _p(out), h * w * c, w * c, MEM_HOST, None))
    return out


def bgr_image_warp_batch_device(src_ptr, n, w, h, c, bits, ts, dst_ptr, mode=WARP_LANCZOS2, border=BORDER_CLAMP,
                                max_value=None, stream=None):
    """device-resident form: dense frames, enqueue only"""
    if max_value is None:
        max_value = 255 if bits == 8 else 65535
    _check(lib().vs_bgr_image_warp_batch(_p(src_ptr), h * w * c, n, w, h, w * c, c, bits, _transforms(ts, n), mode, border, max_value,
                                         _p(dst_ptr), h * w * c, w * c, MEM_DEVICE, _stream(stream)))


def bgr_image_warp_roi_batch(src, ts, roi, mode=WARP_LANCZOS2, border=BORDER_CLAMP, max_value=None):
    """only the window roi = (x, y, w, h) of every warped frame: (n, roi_h, roi_w, c)"""
    src = np.ascontiguousarray(src)
    n, h, w, c = src.shape
    bits, max_value = _depth(src.dtype, max_value)
    rx, ry, rw, rh = roi
    out = np.empty((n, rh, rw, c), src.dtype)
    _check(lib().vs_bgr_image_warp_roi_batch(_p(src), h * w * c, n, w, h, w * c, c, bits, _transforms(ts, n), mode, border, max_value,
                                             rx, ry, rw, rh, _p(out), rh * rw * c, rw * c, MEM_HOST, None))
    return out


# ---- border fill: the fill, its seam blend (channel sums), the coverage index, the inpaint ----
def bgr_image_warp_fill_batch(src, cand_frame, cand_t, roi=None, border=BORDER_CONSTANT, max_value=None, src_stride=None, dst_stride=None):
    """VS_WARP_BILINEAR_CV with border fill (include/vs_amd.h: vs_bgr_image_warp_fill_batch).  src (n_src,h,w,3) numpy; cand_frame
    (n_out, n_cand) ints, a negative index ends a list; cand_t: n_out lists of n_cand Transforms.  -> (n_out, roi_h, roi_w, 3).
    src_stride / dst_stride (elements): the call is made on pitched copies of the frames (the padding is not part of the result)"""
    src, _, ss, buf = _frames_in(src, None, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    n_src, h, w, c = src.shape
    bits, max_value = _depth(src.dtype, max_value)
    rx, ry, rw, rh = _window(roi, w, h)
    out, ds = _frames_out(n_out, rh, rw, c, src.dtype, dst_stride)
    _check(lib().vs_bgr_image_warp_fill_batch(_p(buf), h * ss, n_src, w, h, ss, c, bits, n_out, n_cand, _i32p(idx),
                                              arr, border, max_value, rx, ry, rw, rh, _p(out), rh * ds, ds, MEM_HOST, None))
    return _cut(out, (n_out, rh, rw, c), None)


def channel_sums_batch(src, fmt=None, src_stride=None):
    """the per-channel sample sums of every frame (include/vs_amd.h: vs_bgr_channel_sums_batch).  src (n,h,w,3) numpy -> (n,3) uint64.
    src_stride (elements): the call is made on pitched copies of the frames"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, h, w, c = src.shape
    out = np.zeros((n, 3), np.uint64)
    _check(lib().vs_bgr_channel_sums_batch(_p(buf), h * ss, n, w, h, ss, fmt, _p(out), MEM_HOST, None))
    return out


def channel_sums_batch_device(src_ptr, src_fs, n, w, h, src_stride, fmt, sums_ptr, stream=None):
    """device-resident form (any base address and pitch, in elements): enqueue only"""
    _check(lib().vs_bgr_channel_sums_batch(_p(src_ptr), src_fs, n, w, h, src_stride, fmt, _p(sums_ptr), MEM_DEVICE, _stream(stream)))


def bgr_image_warp_fill_blend_batch(src, cand_frame, cand_t, sums=None, feather=0, match=0, roi=None, border=BORDER_CONSTANT, max_value=None,
                                    src_stride=None, dst_stride=None, guard=None):
    """the fill with its seams blended (include/vs_amd.h: vs_bgr_image_warp_fill_blend_batch).  Arguments as bgr_image_warp_fill_batch;
    sums (n_src,3) uint64 (None only with match == 0).  guard: a value the destination's padding is filled with first; the padded buffer
    is returned as well, so that the caller can see that the padding was left alone"""
    src, _, ss, buf = _frames_in(src, None, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    n_src, h, w, c = src.shape
    bits, max_value = _depth(src.dtype, max_value)
    rx, ry, rw, rh = _window(roi, w, h)
    sm = _c(sums, np.uint64) if sums is not None else None
    p = FillBlendParams(int(feather), int(match))
    out, ds = _frames_out(n_out, rh, rw, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_image_warp_fill_blend_batch(_p(buf), h * ss, n_src, w, h, ss, c, bits, n_out, n_cand, _i32p(idx),
                                                    arr, _p(sm) if sm is not None else None, C.byref(p), border, max_value, rx, ry, rw, rh, _p(out),
                                                    rh * ds, ds, MEM_HOST, None))
    return _cut(out, (n_out, rh, rw, c), guard)


def bgr_fill_coverage_batch(w, h, cand_frame, cand_t, roi=None, cov_stride=None, guard=None):
    """the inpaint's coverage index (include/vs_amd.h: vs_bgr_fill_coverage_batch).  cand_frame (n_out, n_cand) ints, a negative index ends a
    list (only the sign is looked at); cand_t: n_out lists of n_cand Transforms.  -> (n_out, roi_h, roi_w) uint8: 1 + the first covering
    candidate, 0 for none.  cov_stride (bytes): the call is made on a pitched buffer.  guard: a value the padding is filled with first; the
    padded buffer is returned as well"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    rx, ry, rw, rh = _window(roi, w, h)
    out, cs = _frames_out(n_out, rh, rw, 1, np.uint8, cov_stride, guard, fill=0xA5)
    _check(lib().vs_bgr_fill_coverage_batch(w, h, n_out, n_cand, _i32p(idx), arr, rx, ry, rw, rh, _p(out), rh * cs, cs,
                                            MEM_HOST, None))
    return _cut(out, (n_out, rh, rw), guard)


def bgr_fill_coverage_batch_device(w, h, cand_frame, cand_t, roi, cov_ptr, cov_fs, cov_stride, stream=None):
    """device-resident form: the index goes to device memory (strides in bytes), enqueue only"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    rx, ry, rw, rh = roi
    _check(lib().vs_bgr_fill_coverage_batch(w, h, n_out, n_cand, _i32p(idx), arr, rx, ry, rw, rh, _p(cov_ptr), cov_fs,
                                            cov_stride, MEM_DEVICE, _stream(stream)))


def bgr_inpaint_batch(img, mask, fmt=None, stride=None, mask_stride=None, guard=None):
    """push-pull inpaint (include/vs_amd.h: vs_bgr_inpaint_batch).  img (n,h,w,3) numpy, mask (n,h,w) bytes (non-zero = keep) -> (n,h,w,3);
    img is not changed.  stride (elements) / mask_stride (bytes): the call is made on pitched buffers.  guard: a value the image's padding is
    filled with first; the padded buffer is returned as well"""
    img = np.ascontiguousarray(img)
    n, h, w, c = img.shape
    fmt = _fmt_of(img.dtype, 3) if fmt is None else fmt
    ms = w if mask_stride is None else mask_stride
    buf, st = _frames_out(n, h, w, c, img.dtype, stride, guard)         # in place: the destination starts as the image
    buf[:n, :, :w * c] = img.reshape(n, h, w * c)
    mk = np.zeros((n, h, ms), np.uint8)
    mk[:, :, :w] = _c(mask, np.uint8).reshape(n, h, w)
    _check(lib().vs_bgr_inpaint_batch(_p(buf), h * st, n, w, h, st, fmt, _p(mk), h * ms, ms, MEM_HOST, None))
    return _cut(buf, (n, h, w, c), guard)


def bgr_inpaint_batch_device(img_ptr, frame_stride, n, w, h, stride, fmt, mask_ptr, mask_fs, mask_stride, stream=None):
    """device-resident form: in place (frame_stride, stride in elements; the mask's in bytes)"""
    _check(lib().vs_bgr_inpaint_batch(_p(img_ptr), frame_stride, n, w, h, stride, fmt, _p(mask_ptr), mask_fs, mask_stride, MEM_DEVICE,
                                      _stream(stream)))


# ---- deblur by transfer (sharpness, then the transfer) ----
def deblur_params(**kw):
    return _params(DeblurParams, "vs_deblur_params_default", kw)


def sharpness_batch(src, fmt=None, src_stride=None):
    """the gradient energy S of every frame (include/vs_amd.h: vs_bgr_sharpness_batch).  src (n,h,w,3) numpy -> (n,) uint64.
    src_stride (elements): the call is made on pitched copies of the frames"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, h, w, c = src.shape
    out = np.zeros(n, np.uint64)
    _check(lib().vs_bgr_sharpness_batch(_p(buf), h * ss, n, w, h, ss, fmt, _p(out), MEM_HOST, None))
    return out


def sharpness_batch_device(src_ptr, n, w, h, fmt, sharp_ptr, stream=None):
    _check(lib().vs_bgr_sharpness_batch(_p(src_ptr), h * w * 3, n, w, h, w * 3, fmt, _p(sharp_ptr), MEM_DEVICE, _stream(stream)))


def bgr_deblur_batch(src, sharpness, cand_frame, cand_t, params=None, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """deblur by transfer (include/vs_amd.h: vs_bgr_deblur_batch).  src (n_src,h,w,3) numpy; sharpness (n_src,) uint64; cand_frame
    (n_out, n_cand) ints, a negative index ends a list; cand_t: n_out lists of n_cand Transforms.  -> (n_out, h, w, 3).
    src_stride / dst_stride (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with
    first; the padded buffer is returned as well, so that the caller can see that the padding was left alone"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    n_src, h, w, c = src.shape
    sh = _c(sharpness, np.uint64)
    out, ds = _frames_out(n_out, h, w, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_deblur_batch(_p(buf), h * ss, n_src, w, h, ss, fmt, _p(sh), n_out, n_cand, _i32p(idx), arr,
                                     _ref(params), _p(out), h * ds, ds, MEM_HOST, None))
    return _cut(out, (n_out, h, w, c), guard)


def bgr_deblur_batch_device(src_ptr, n_src, w, h, fmt, sharp_ptr, cand_frame, cand_t, dst_ptr, params=None, stream=None):
    """device-resident form: dense frames, sharpness in device memory, enqueue only"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    _check(lib().vs_bgr_deblur_batch(_p(src_ptr), h * w * 3, n_src, w, h, w * 3, fmt, _p(sharp_ptr), n_out, n_cand,
                                     _i32p(idx), arr, _ref(params), _p(dst_ptr), h * w * 3, w * 3, MEM_DEVICE, _stream(stream)))


# ---- motion-compensated temporal denoise ----
def denoise_params(**kw):
    return _params(DenoiseParams, "vs_denoise_params_default", kw)


def denoise_batch(src, cand_frame, cand_t, params=None, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """motion-compensated temporal denoise (include/vs_amd.h: vs_bgr_denoise_batch).  src (n_src,h,w,3) numpy; cand_frame (n_out, n_cand)
    ints, a negative index ends a list; cand_t: n_out lists of n_cand Transforms.  -> (n_out, h, w, 3).  src_stride / dst_stride
    (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with first; the padded buffer
    is returned as well, so that the caller can see that the padding was left alone"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    n_src, h, w, c = src.shape
    out, ds = _frames_out(n_out, h, w, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_denoise_batch(_p(buf), h * ss, n_src, w, h, ss, fmt, n_out, n_cand, _i32p(idx), arr,
                                      _ref(params), _p(out), h * ds, ds, MEM_HOST, None))
    return _cut(out, (n_out, h, w, c), guard)


def denoise_batch_device(src_ptr, src_fs, n_src, w, h, src_stride, fmt, cand_frame, cand_t, dst_ptr, dst_fs, dst_stride, params=None, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    _check(lib().vs_bgr_denoise_batch(_p(src_ptr), src_fs, n_src, w, h, src_stride, fmt, n_out, n_cand, _i32p(idx), arr,
                                      _ref(params), _p(dst_ptr), dst_fs, dst_stride, MEM_DEVICE, _stream(stream)))


# ---- rolling-shutter correction ----
def rolling_params(**kw):
    return _params(RollingParams, "vs_rolling_params_default", kw)


def rolling_batch(src, cand_frame, cand_t, params=None, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """rolling-shutter correction (include/vs_amd.h: vs_bgr_rolling_batch).  src (n_src,h,w,3) numpy; cand_frame (n_out, 2) ints: the frame,
    then any index >= 0 (a motion is known) or a negative one (none); cand_t: n_out lists of 2 Transforms, the second the motion to the
    following frame.  -> (n_out, h, w, 3).  src_stride / dst_stride (elements): the call is made on pitched buffers.  guard: a value the
    destination's padding is filled with first; the padded buffer is returned as well"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    assert n_cand == 2
    n_src, h, w, c = src.shape
    out, ds = _frames_out(n_out, h, w, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_rolling_batch(_p(buf), h * ss, n_src, w, h, ss, fmt, n_out, _i32p(idx), arr,
                                      _ref(params), _p(out), h * ds, ds, MEM_HOST, None))
    return _cut(out, (n_out, h, w, c), guard)


def rolling_batch_device(src_ptr, src_fs, n_src, w, h, src_stride, fmt, cand_frame, cand_t, dst_ptr, dst_fs, dst_stride, params=None, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    assert n_cand == 2
    _check(lib().vs_bgr_rolling_batch(_p(src_ptr), src_fs, n_src, w, h, src_stride, fmt, n_out, _i32p(idx), arr,
                                      _ref(params), _p(dst_ptr), dst_fs, dst_stride, MEM_DEVICE, _stream(stream)))


# ---- lens-distortion correction: the radial map, the remap through it ----
REMAP_SLICE = 8                                     # vsk::kRemapSlice: the frames a workgroup of the remap takes a pixel through


def lens_params(w, h, **kw):
    """the identity lens of a w x h frame (vs_lens_params_default), fields overridden by keyword"""
    return _params(LensParams, "vs_lens_params_default", kw, int(w), int(h))


def lens_map(params, w, h, map_stride=None, guard=None):
    """the radial map on the host (include/vs_amd.h: vs_lens_map, VS_MEM_HOST: no device needed) -> (h, w, 2) int32 positions (X, Y) with 5
    fraction bits.  map_stride (int32 elements): the map is made in pitched rows.  guard: a value the buffer -- two rows in front, two behind and
    the padding -- is filled with first; the whole buffer (h + 4, map_stride) is returned as well"""
    ms = 2 * w if map_stride is None else map_stride
    buf = np.full((h + 4, ms), 0 if guard is None else guard, np.int32)
    _check(lib().vs_lens_map(C.byref(params), w, h, _p(buf[2:]), ms, MEM_HOST, None))
    res = np.ascontiguousarray(buf[2:h + 2, :2 * w]).reshape(h, w, 2)
    return (res, buf) if guard is not None else res


def lens_map_device(params, w, h, map_ptr, map_stride=None, stream=None):
    """device-resident form: the map is written at map_ptr (int32, rows of map_stride elements), enqueue only"""
    _check(lib().vs_lens_map(C.byref(params), w, h, _p(map_ptr), 2 * w if map_stride is None else map_stride, MEM_DEVICE, _stream(stream)))


def remap_batch(src, pos, border=BORDER_CLAMP, fmt=None, src_stride=None, dst_stride=None, map_stride=None, guard=None):
    """remap through a map of fixed-point positions (include/vs_amd.h: vs_bgr_remap_batch).  src (n,h,w,3) numpy; pos (oh, ow, 2) int32 (X, Y)
    with 5 fraction bits, one map for every frame -> (n, oh, ow, 3).  src_stride / dst_stride (elements), map_stride (int32 elements): the call
    is made on pitched buffers.  guard: a value the destination's padding is filled with first; the padded buffer is returned as well"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, h, w, c = src.shape
    pos = _c(pos, np.int32)
    oh, ow, _ = pos.shape
    ms = 2 * ow if map_stride is None else map_stride
    mp = _pitched(pos.reshape(1, oh, ow, 2), ms)
    out, ds = _frames_out(n, oh, ow, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_remap_batch(_p(buf), h * ss, n, w, h, ss, fmt, _p(mp), ms, ow, oh, border, _p(out), oh * ds, ds, MEM_HOST, None))
    return _cut(out, (n, oh, ow, c), guard)


def remap_batch_device(src_ptr, src_fs, n, w, h, src_stride, fmt, map_ptr, map_stride, ow, oh, dst_ptr, dst_fs, dst_stride, border=BORDER_CLAMP, stream=None):
    """device-resident form: frames and map in device memory, frame strides and row strides in elements, enqueue only"""
    _check(lib().vs_bgr_remap_batch(_p(src_ptr), src_fs, n, w, h, src_stride, fmt, _p(map_ptr), map_stride, ow, oh, border, _p(dst_ptr), dst_fs, dst_stride,
                                    MEM_DEVICE, _stream(stream)))


# ---- resize (include/vs_amd.h: THE RESIZE RULE; the tables: csrc/vs_resize.hpp) ----
def resize_taps(s, d, filter=RESIZE_LINEAR):
    """one axis' tap table on the host (include/vs_amd.h: vs_resize_taps, no device needed) -> (i0 (d,), n (d,), wt (d, 10) uint16)"""
    i0, n, wt = np.zeros(max(d, 1), np.int32), np.zeros(max(d, 1), np.int32), np.zeros((max(d, 1), 10), np.uint16)
    _check(lib().vs_resize_taps(int(s), int(d), int(filter), _p(i0), _p(n), _p(wt)))
    return i0, n, wt


def resize_batch(src, dw, dh, filter=RESIZE_LINEAR, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """resize by THE RESIZE RULE (include/vs_amd.h: vs_bgr_resize_batch).  src (n,sh,sw,3) numpy -> (n, dh, dw, 3).  src_stride / dst_stride
    (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with first; the padded buffer is
    returned as well"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, sh, sw, c = src.shape
    out, ds = _frames_out(n, dh, dw, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_resize_batch(_p(buf), sh * ss, n, sw, sh, ss, fmt, int(filter), _p(out), dh * ds, dw, dh, ds, MEM_HOST, None))
    return _cut(out, (n, dh, dw, c), guard)


def resize_batch_device(src_ptr, src_fs, n, sw, sh, src_stride, fmt, filter, dst_ptr, dst_fs, dw, dh, dst_stride, stream=None):
    """device-resident form: frames in device memory, frame strides and row strides in elements, enqueue only"""
    _check(lib().vs_bgr_resize_batch(_p(src_ptr), src_fs, n, sw, sh, src_stride, fmt, int(filter), _p(dst_ptr), dst_fs, dw, dh, dst_stride, MEM_DEVICE,
                                     _stream(stream)))


# ---- YCbCr frames (include/vs_amd.h: vs_ycbcr_to_bgr_batch; the rule: csrc/vs_ycbcr.hpp) ----
def chroma_shape(w, h, sub):
    """(cw, ch) of a w x h frame's chroma planes under sub = (sub_x, sub_y)"""
    return (w + sub[0]) >> sub[0], (h + sub[1]) >> sub[1]


def ycbcr_planes(y, cb, cr, y_stride, c_stride, c_step, sub, y_frame_stride, c_frame_stride):
    """a vs_ycbcr_planes from raw addresses (ints; cb = cr = None: luma only), strides in elements"""
    vp = (lambda a: None if a is None else C.c_void_p(int(a)))
    return YcbcrPlanes(vp(y), vp(cb), vp(cr), int(y_stride), int(c_stride), int(c_step), int(sub[0]), int(sub[1]), int(y_frame_stride), int(c_frame_stride))


class _HostPlanes:
    """the planes of n frames in host buffers of their own, as the host forms below lay them out: Y rows of y_stride elements; chroma planar
    (two buffers, rows of c_stride) or, interleaved = "nv12" (Cb first) / "nv21" (Cr first), one buffer of pairs.  Every buffer has two guard
    rows in front and two behind; `fill` is what buffers and padding start with.  desc: the vs_ycbcr_planes of it"""

    def __init__(self, n, w, h, dtype, sub, interleaved, mono, y_stride, c_stride, fill):
        cw, ch = chroma_shape(w, h, sub)
        self.n, self.w, self.h, self.cw, self.ch, self.sub, self.interleaved, self.mono = n, w, h, cw, ch, sub, interleaved, mono
        step = 2 if interleaved else 1
        self.ys = w if y_stride is None else y_stride
        self.cs = cw * step if c_stride is None else c_stride
        self.ybuf = np.full((n * h + 4, self.ys), fill, dtype)
        self.cbufs = [] if mono else [np.full((n * ch + 4, self.cs), fill, dtype) for _ in range(1 if interleaved else 2)]
        esz = np.dtype(dtype).itemsize
        ya = self.ybuf[2:].ctypes.data
        if mono:
            ca = ra = None
        elif interleaved:
            base = self.cbufs[0][2:].ctypes.data
            ca, ra = (base, base + esz) if interleaved == "nv12" else (base + esz, base)
        else:
            ca, ra = self.cbufs[0][2:].ctypes.data, self.cbufs[1][2:].ctypes.data
        self.desc = ycbcr_planes(ya, ca, ra, self.ys, self.cs, step, sub, h * self.ys, ch * self.cs)

    def _views(self):
        n, w, h, cw, ch = self.n, self.w, self.h, self.cw, self.ch
        yv = self.ybuf[2:2 + n * h].reshape(n, h, self.ys)[:, :, :w]
        if self.mono:
            return yv, None, None
        if self.interleaved:
            pairs = self.cbufs[0][2:2 + n * ch].reshape(n, ch, self.cs)[:, :, :2 * cw]
            first, second = pairs[:, :, 0::2], pairs[:, :, 1::2]
            return (yv, first, second) if self.interleaved == "nv12" else (yv, second, first)
        return (yv,) + tuple(b[2:2 + n * ch].reshape(n, ch, self.cs)[:, :, :cw] for b in self.cbufs)

    def put(self, y, cb, cr):
        yv, cbv, crv = self._views()
        yv[...] = y
        if not self.mono:
            cbv[...] = cb
            crv[...] = cr

    def get(self):
        return tuple(None if v is None else np.ascontiguousarray(v) for v in self._views())

    def buffers(self):
        return [self.ybuf] + self.cbufs


def ycbcr_to_bgr_batch(y, cb=None, cr=None, sub=(1, 1), fmt=None, interleaved=None, y_stride=None, c_stride=None, dst_stride=None, guard=None):
    """YCbCr planes -> interleaved BGR (include/vs_amd.h: vs_ycbcr_to_bgr_batch).  y (n,h,w) numpy; cb, cr (n,ch,cw) or both None (luma only);
    sub = (sub_x, sub_y): log2 subsampling; interleaved: None (planar), "nv12" or "nv21" (the chroma travels as one plane of pairs) -> (n,h,w,3).
    y_stride / c_stride / dst_stride (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with
    first; the padded buffer is returned as well"""
    y = np.ascontiguousarray(y)
    n, h, w = y.shape
    fmt = _fmt_of(y.dtype, 3) if fmt is None else fmt
    hp = _HostPlanes(n, w, h, y.dtype, sub, interleaved, cb is None, y_stride, c_stride, 0)
    hp.put(y, cb, cr)
    out, ds = _frames_out(n, h, w, 3, y.dtype, dst_stride, guard)
    _check(lib().vs_ycbcr_to_bgr_batch(C.byref(hp.desc), n, w, h, fmt, _p(out), h * ds, ds, MEM_HOST, None))
    return _cut(out, (n, h, w, 3), guard)


def ycbcr_to_bgr_batch_device(planes, n, w, h, fmt, dst_ptr, dst_fs, dst_stride, stream=None):
    """device-resident form: planes is a YcbcrPlanes of device addresses (ycbcr_planes), strides in elements, enqueue only"""
    _check(lib().vs_ycbcr_to_bgr_batch(C.byref(planes), n, w, h, fmt, _p(dst_ptr), dst_fs, dst_stride, MEM_DEVICE, _stream(stream)))


def bgr_to_ycbcr_batch(src, sub=(1, 1), fmt=None, interleaved=None, mono=False, src_stride=None, y_stride=None, c_stride=None, guard=None):
    """interleaved BGR -> YCbCr planes (include/vs_amd.h: vs_bgr_to_ycbcr_batch).  src (n,h,w,3) numpy -> (y (n,h,w), cb, cr (n,ch,cw)); mono:
    luma only, cb and cr come back None.  Strides in elements: the call is made on pitched buffers.  guard: a value the destination buffers --
    two rows in front, two behind and the padding -- are filled with first; the whole buffers are returned as well, as a list"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, h, w, c = src.shape
    hp = _HostPlanes(n, w, h, src.dtype, sub, interleaved, mono, y_stride, c_stride, 0 if guard is None else guard)
    _check(lib().vs_bgr_to_ycbcr_batch(_p(buf), h * ss, n, w, h, ss, fmt, C.byref(hp.desc), MEM_HOST, None))
    return (hp.get(), hp.buffers()) if guard is not None else hp.get()


def bgr_to_ycbcr_batch_device(src_ptr, src_fs, n, w, h, src_stride, fmt, planes, stream=None):
    """device-resident form: frames and planes (a YcbcrPlanes of device addresses) in device memory, strides in elements, enqueue only"""
    _check(lib().vs_bgr_to_ycbcr_batch(_p(src_ptr), src_fs, n, w, h, src_stride, fmt, C.byref(planes), MEM_DEVICE, _stream(stream)))


# ---- deflicker: pair statistics, gains from them, the point-wise gain pass ----
def deflicker_params(**kw):
    return _params(DeflickerParams, "vs_deflicker_params_default", kw)


def exposure_stats_batch(src, cand_frame, cand_t, params=None, fmt=None, src_stride=None):
    """the deflicker's pair statistics (include/vs_amd.h: vs_bgr_exposure_stats_batch).  src (n_src,h,w,3) numpy; cand_frame (n_out, n_cand) ints,
    a negative index ends a list; cand_t: n_out lists of n_cand Transforms.  -> (n_out, n_cand, 8) uint64.  src_stride (elements): the call is
    made on pitched copies of the frames"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    n_src, h, w, c = src.shape
    out = np.full((max(n_out, 1), max(n_cand, 1), 8), 0xA5A5A5A5, np.uint64)
    _check(lib().vs_bgr_exposure_stats_batch(_p(buf), h * ss, n_src, w, h, ss, fmt, n_out, n_cand, _i32p(idx), arr,
                                             _ref(params), _p(out), MEM_HOST, None))
    return out


def exposure_stats_batch_device(src_ptr, src_fs, n_src, w, h, src_stride, fmt, cand_frame, cand_t, stats_ptr, params=None, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    idx, n_out, n_cand, arr = _candidates(cand_frame, cand_t)
    _check(lib().vs_bgr_exposure_stats_batch(_p(src_ptr), src_fs, n_src, w, h, src_stride, fmt, n_out, n_cand, _i32p(idx),
                                             arr, _ref(params), _p(stats_ptr), MEM_DEVICE, _stream(stream)))


def exposure_gains_batch(stats, w, h, params=None):
    """the deflicker's gains from its statistics (include/vs_amd.h: vs_exposure_gains_batch).  stats (n_out, n_cand, 8) uint64 -> (n_out, 4)
    uint32: G_B, G_G, G_R, m"""
    st = _c(stats, np.uint64)
    n_out, n_cand = st.shape[0], st.shape[1]
    out = np.full((n_out, 4), 0xA5A5A5A5, np.uint32)
    _check(lib().vs_exposure_gains_batch(_p(st), n_out, n_cand, w, h, _ref(params), _p(out), MEM_HOST, None))
    return out


def exposure_gains_batch_device(stats_ptr, n_out, n_cand, w, h, gains_ptr, params=None, stream=None):
    _check(lib().vs_exposure_gains_batch(_p(stats_ptr), n_out, n_cand, w, h, _ref(params), _p(gains_ptr), MEM_DEVICE, _stream(stream)))


def bgr_gain_batch(src, gains, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """the deflicker's point-wise pass (include/vs_amd.h: vs_bgr_gain_batch).  src (n,h,w,3) numpy; gains (n,4) uint32 -> (n,h,w,3).  src_stride /
    dst_stride (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with first; the padded
    buffer is returned as well"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, h, w, c = src.shape
    g = _c(gains, np.uint32)
    out, ds = _frames_out(n, h, w, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_gain_batch(_p(buf), h * ss, n, w, h, ss, fmt, _p(g), _p(out), h * ds, ds, MEM_HOST, None))
    return _cut(out, (n, h, w, c), guard)


def bgr_gain_batch_device(src_ptr, src_fs, n, w, h, src_stride, fmt, gains_ptr, dst_ptr, dst_fs, dst_stride, stream=None):
    """device-resident form (dst_ptr may equal src_ptr): enqueue only"""
    _check(lib().vs_bgr_gain_batch(_p(src_ptr), src_fs, n, w, h, src_stride, fmt, _p(gains_ptr), _p(dst_ptr), dst_fs, dst_stride, MEM_DEVICE,
                                   _stream(stream)))


# ---- scene-cut detection: pair statistics, the rule's decision ----
def scene_params(**kw):
    return _params(SceneParams, "vs_scene_params_default", kw)


def _scene_pairs(pair_frames, pair_t):
    """_pairs, and one Transform for every pair"""
    idx, n_pairs = _pairs(pair_frames)
    assert len(pair_t) == n_pairs
    return idx, n_pairs, _transforms(pair_t, n_pairs)


def scene_stats_batch(src, pair_frames, pair_t, params=None, fmt=None, src_stride=None):
    """the scene-cut pair statistics (include/vs_amd.h: vs_bgr_scene_stats_batch).  src (n_src,h,w,3) numpy; pair_frames (n_pairs, 2) ints: target,
    candidate; pair_t: n_pairs Transforms.  -> (n_pairs, 2) uint64: count, sad.  src_stride (elements): the call is made on pitched copies of the
    frames"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n_src, h, w, c = src.shape
    idx, n_pairs, arr = _scene_pairs(pair_frames, pair_t)
    out = np.full((max(n_pairs, 1), 2), 0xA5A5A5A5, np.uint64)
    _check(lib().vs_bgr_scene_stats_batch(_p(buf), h * ss, n_src, w, h, ss, fmt, n_pairs, _i32p(idx), arr,
                                          _ref(params), _p(out), MEM_HOST, None))
    return out[:n_pairs]


def scene_stats_batch_device(src_ptr, src_fs, n_src, w, h, src_stride, fmt, pair_frames, pair_t, stats_ptr, params=None, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    idx, n_pairs, arr = _scene_pairs(pair_frames, pair_t)
    _check(lib().vs_bgr_scene_stats_batch(_p(src_ptr), src_fs, n_src, w, h, src_stride, fmt, n_pairs, _i32p(idx), arr,
                                          _ref(params), _p(stats_ptr), MEM_DEVICE, _stream(stream)))


def scene_cuts(stats, w, h, params=None):
    """the scene-cut rule's decision, on the host (include/vs_amd.h: vs_scene_cuts).  stats (n_pairs, 2) uint64 -> (n_pairs,) uint8"""
    st = _c(stats, np.uint64).reshape(-1, 2)
    out = np.full((max(st.shape[0], 1),), 0xA5, np.uint8)
    _check(lib().vs_scene_cuts(_p(st), st.shape[0], w, h, _ref(params), _p(out)))
    return out[:st.shape[0]]


# ---- fidelity metrics: pair statistics, the rule's scores ----
def fidelity_stats_batch(a, b, pair_frames, fmt=None, a_stride=None, b_stride=None, roi=None):
    """the fidelity statistics of image pairs (include/vs_amd.h: vs_bgr_fidelity_batch).  a (n_a,h,w,3) and b (n_b,h,w,3) numpy of one dtype; b None
    or a itself: the pairs lie in one batch, handed over once; pair_frames (n_pairs, 2) ints: into a, into b.  -> (n_pairs, 6) uint64: sse_b, sse_g,
    sse_r, sse_y, n_win, ssim_sum (two's complement).  a_stride / b_stride (elements): the call is made on pitched copies of the frames.  roi
    (x, y, rw, rh): the images are that window of the frames, handed over as its origin pointer with the frames' strides"""
    a, fmt, sa, pa = _frames_in(a, fmt, a_stride)
    one = b is None or b is a
    if one and b_stride in (None, sa):
        b, sb, pb = a, sa, pa
    else:
        b, _, sb, pb = _frames_in(a if one else b, fmt, b_stride)
    assert a.dtype == b.dtype and a.shape[1:] == b.shape[1:]
    n_a, h, w, c = a.shape
    idx, n_pairs = _pairs(pair_frames)
    x, y, rw, rh = _window(roi, w, h)
    assert 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
    esz = a.dtype.itemsize
    out = np.full((max(n_pairs, 1), 6), 0xA5A5A5A5, np.uint64)
    _check(lib().vs_bgr_fidelity_batch(C.c_void_p(pa.ctypes.data + (y * sa + x * c) * esz), h * sa, n_a, sa,
                                       C.c_void_p(pb.ctypes.data + (y * sb + x * c) * esz), h * sb, b.shape[0], sb, rw, rh, fmt, n_pairs,
                                       _i32p(idx), _p(out), MEM_HOST, None))
    return out[:n_pairs]


def fidelity_stats_batch_device(a_ptr, a_fs, n_a, a_stride, b_ptr, b_fs, n_b, b_stride, w, h, fmt, pair_frames, stats_ptr, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    idx, n_pairs = _pairs(pair_frames)
    _check(lib().vs_bgr_fidelity_batch(_p(a_ptr), a_fs, n_a, a_stride, _p(b_ptr), b_fs, n_b, b_stride, w, h, fmt, n_pairs,
                                       _i32p(idx), _p(stats_ptr), MEM_DEVICE, _stream(stream)))


def fidelity_scores(stats, w, h, fmt=FMT_BGR8):
    """the fidelity rule's scores, on the host (include/vs_amd.h: vs_fidelity_scores).  stats (n_pairs, 6) uint64 -> (n_pairs, 6) float64: psnr_b,
    psnr_g, psnr_r, psnr, psnr_y, ssim"""
    st = _c(stats, np.uint64).reshape(-1, 6)
    n = st.shape[0]
    arr = (FidelityScore * max(n, 1))()
    _check(lib().vs_fidelity_scores(_p(st), n, w, h, fmt, arr))
    return np.array([arr[i].tup() for i in range(n)], np.float64).reshape(n, 6)


# ---- phase-compensated sharpening ----
def sharpen_params(**kw):
    return _params(SharpenParams, "vs_sharpen_params_default", kw)


def sharpen_batch(src, ts, w, h, roi_x=0, roi_y=0, params=None, fmt=None, src_stride=None, dst_stride=None, guard=None):
    """phase-compensated sharpening behind VS_WARP_BILINEAR_CV (include/vs_amd.h: vs_bgr_sharpen_batch).  src (n, roi_h, roi_w, 3) numpy: the
    window at (roi_x, roi_y) of w x h output frames warped under the forward Transforms ts (n of them) -> (n, roi_h, roi_w, 3).  src_stride /
    dst_stride (elements): the call is made on pitched buffers.  guard: a value the destination's padding is filled with first; the padded
    buffer is returned as well"""
    src, fmt, ss, buf = _frames_in(src, fmt, src_stride)
    n, rh, rw, c = src.shape
    assert len(ts) == n
    out, ds = _frames_out(n, rh, rw, c, src.dtype, dst_stride, guard)
    _check(lib().vs_bgr_sharpen_batch(_p(buf) if n else None, rh * ss, n, w, h, fmt, _transforms(ts, n), _ref(params),
                                      roi_x, roi_y, rw, rh, ss, _p(out), rh * ds, ds, MEM_HOST, None))
    return _cut(out, (n, rh, rw, c), guard)


def sharpen_batch_device(src_ptr, src_fs, n, w, h, fmt, ts, roi_x, roi_y, roi_w, roi_h, src_stride, dst_ptr, dst_fs, dst_stride, params=None, stream=None):
    """device-resident form: frame strides and row strides in elements, enqueue only"""
    _check(lib().vs_bgr_sharpen_batch(_p(src_ptr), src_fs, n, w, h, fmt, _transforms(ts, n), _ref(params), roi_x, roi_y, roi_w, roi_h,
                                      src_stride, _p(dst_ptr), dst_fs, dst_stride, MEM_DEVICE, _stream(stream)))


# ---- engine level ---------------------------------------------------------------------------
def _dense(w, h, fmt, stride, frame_stride):
    """the strides (elements) of device-resident frames: dense unless the caller says otherwise"""
    stride = stride or w * _channels(fmt)
    return stride, frame_stride or h * stride


def _batch_outs(n):
    """the out-arguments of a process_* call over n frames: has_output, out_w, out_h"""
    return (C.c_int32 * n)(), C.c_int(), C.c_int()


# ---- dense optical flow (this build's Farneback specification, vs_flow.hip) -------------------
def flow_params(**kw):
    """FlowParams with the reference's defaults (0.5, 3, 15, 3, 5, 1.2, 0), fields overridden by keyword"""
    return _params(FlowParams, "vs_flow_params_default", kw)


class Flow(_Handle):
    """a vs_flow handle: its own stream and scratch, reused by every call"""
    _create, _destroy = "vs_flow_create", "vs_flow_destroy"

    def __init__(self, params=None, device=0):
        self.params = params if params is not None else flow_params()
        self._open(C.byref(self.params), device)

    def compute(self, prev, next_):
        """(h, w, 2) float32 flow (dx, dy) from prev to next (u8 gray, or any 2-D array with row stride = its strides[0])"""
        a = np.asarray(prev)
        b = np.asarray(next_)
        if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 2 or a.shape != b.shape:
            raise ValueError("dense_flow takes two u8 gray images of the same shape")
        if a.strides[1] != 1 or b.strides[1] != 1 or a.strides[0] != b.strides[0]:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        h, w = a.shape
        out = np.empty((h, w, 2), np.float32)
        _check(lib().vs_flow_compute(self.h, _p(a), _p(b), w, h, a.strides[0], MEM_HOST, _p(out), 2 * w))
        return out

    def _jitter(self, ptr, frame_stride, n, w, h, stride, fmt, mem):
        pm = np.zeros(max(n - 1, 0), np.float32)
        med = C.c_double(0.0)
        _check(lib().vs_flow_jitter(self.h, _p(ptr), frame_stride, n, w, h, stride, fmt, mem, _p(pm), C.byref(med)))
        return med.value, pm

    def jitter(self, frames, fmt=None):
        """frames: numpy (n, h, w) u8 gray or (n, h, w, 3) BGR u8 / u16 (10-bit unless fmt says otherwise).
        returns (median, pair medians (n-1) float32)"""
        frames = np.ascontiguousarray(frames)
        fmt = _fmt_of(frames.dtype, frames.ndim - 1) if fmt is None else fmt
        n, hh, ww = frames.shape[:3]
        ch = _channels(fmt)
        return self._jitter(frames, hh * ww * ch, n, ww, hh, ww * ch, fmt, MEM_HOST)

    def jitter_device(self, ptr, n, w, h, fmt, stride=None, frame_stride=None):
        """device-resident frames (raw device pointer; strides in elements): (median, pair medians)"""
        stride, frame_stride = _dense(w, h, fmt, stride, frame_stride)
        return self._jitter(ptr, frame_stride, n, w, h, stride, fmt, MEM_DEVICE)


def dense_flow(prev, next_, params=None, device=0):
    """cv::calcOpticalFlowFarneback(prev, next, flow, ...) under this build's specification: (h, w, 2) float32 (dx, dy)"""
    return Flow(params, device).compute(prev, next_)


def flow_jitter(frames, params=None, fmt=None, device=0):
    """the reference's jitter score of a clip (eval_jitter.cpp:43-70): (median over pairs, per-pair medians)"""
    return Flow(params, device).jitter(frames, fmt)


# ---- the aligner -----------------------------------------------------------------------------
def aligner_params(**kw):
    return _params(AlignerParams, "vs_aligner_params_default", kw)


class Aligner(_Handle):
    """VideoAligner (alignment.hpp:51-99) on the GPU engine."""
    _create, _destroy = "vs_aligner_create", "vs_aligner_destroy"

    def __init__(self, device=0, select_mode=SELECT_DEVICE, **params):
        self.params = aligner_params(**params)
        self._open(C.byref(self.params), device)
        _check(lib().vs_aligner_set_select_mode(self.h, select_mode))

    def set_select_mode(self, mode):
        """SELECT_DEVICE (default: libstdc++'s nth_element order, replicated on the device), SELECT_STABLE (the documented
        STL-independent rule: smallest by (abs_delta, tile index), survivors in tile order) or SELECT_STL_HOST"""
        _check(lib().vs_aligner_set_select_mode(self.h, mode))

    def select_mode(self):
        """the selection mode in force (the VS_SELECT_MODE environment override included)"""
        return _check(lib().vs_aligner_get_select_mode(self.h))

    def set_batch_mode(self, mode):
        """BATCH_SHARED: full batches run through the small-footprint solver kernel (same bits; for callers that overlap
        other GPU work, e.g. the previous clip's warp)"""
        _check(lib().vs_aligner_set_batch_mode(self.h, mode))

    def align_next(self, frame, fmt=None):
        """frame: numpy (h,w) u8 gray, (h,w,3) u8/u16 BGR (u16 = 10-bit unless fmt says FMT_BGR12 / FMT_BGR16_FULL).
        returns (ok, Transform)"""
        frame = np.ascontiguousarray(frame)
        fmt = _fmt_of(frame.dtype, frame.ndim) if fmt is None else fmt
        hh, ww = frame.shape[:2]
        t = Transform()
        r = _check(lib().vs_aligner_align_next(self.h, _p(frame), ww, hh, ww * _channels(fmt), fmt, MEM_HOST, C.byref(self.params), C.byref(t)))
        return bool(r), t

    def _align(self, entry, n, raw, *args):
        """one batched call: `args` lie between the handle and the parameters; -> (status, transforms), as ctypes arrays if raw"""
        out = (Transform * n)()
        status = (C.c_int32 * n)()
        _check(getattr(lib(), entry)(self.h, *args, C.byref(self.params), out, status))
        if raw:
            return status, out       # ctypes arrays: no per-frame Python objects (bench.py hands `out` to the warp call)
        return list(status), list(out)

    def align_batch(self, frames, fmt=None):
        """frames: numpy (n,h,w[,3]).  returns (status[n], [Transform]*n)"""
        frames = np.ascontiguousarray(frames)
        fmt = _fmt_of(frames.dtype, frames.ndim - 1) if fmt is None else fmt
        n, hh, ww = frames.shape[:3]
        ch = _channels(fmt)
        return self._align("vs_aligner_align_batch", n, False, _p(frames), hh * ww * ch, n, ww, hh, ww * ch, fmt, MEM_HOST)

    def align_batch_device(self, ptr, n, w, h, fmt, stride=None, frame_stride=None):
        """device-resident frames (raw device pointer)"""
        stride, frame_stride = _dense(w, h, fmt, stride, frame_stride)
        return self._align("vs_aligner_align_batch", n, False, _p(ptr), frame_stride, n, w, h, stride, fmt, MEM_DEVICE)

    def align_clips(self, frames, n_clips, mem_ptr=None, w=None, h=None, fmt=None, raw=False):
        """frames: numpy (n_clips*fpc, h, w[,3]) (host) -- or pass mem_ptr/w/h/fmt with frames = total frame count
        for dense device-resident clips.  returns (status list, transforms list)"""
        if mem_ptr is None:
            frames = np.ascontiguousarray(frames)
            n = frames.shape[0]
            fmt = _fmt_of(frames.dtype, frames.ndim - 1) if fmt is None else fmt
            h, w = frames.shape[1:3]
            ptr, mem = _p(frames), MEM_HOST
        else:
            n, ptr, mem = int(frames), _p(mem_ptr), MEM_DEVICE
        ch = _channels(fmt)
        return self._align("vs_aligner_align_clips", n, raw, ptr, h * w * ch, n_clips, n // n_clips, w, h, w * ch, fmt, mem)

    def reset(self):
        _check(lib().vs_aligner_reset(self.h))

    def enable_timing(self, on=True):
        _check(lib().vs_aligner_enable_timing(self.h, 1 if on else 0))

    def timings(self):
        t = StageTimings()
        _check(lib().vs_aligner_get_timings(self.h, C.byref(t)))
        d = {name: {"ms": t.ms[i], "launches": t.launches[i]} for i, name in enumerate(STAGES)}
        d["frames"] = t.frames
        d["gn_iterations"] = t.gn_iterations
        return d

    def wait_stream(self, stream_handle):
        """order the handle's stream behind everything enqueued so far on the caller's stream (raw hipStream_t value)"""
        _check(lib().vs_aligner_wait_stream(self.h, C.c_void_p(stream_handle)))

    def info(self, i=0):
        inf = AlignInfo()
        _check(lib().vs_aligner_get_info(self.h, i, C.byref(inf)))
        return inf

    def _level_dims(self, level):
        dims = [C.c_int() for _ in range(5)]
        _check(lib().vs_aligner_level_dims(self.h, level, *(C.byref(v) for v in dims)))
        return dict(zip(("w", "h", "tx", "ty", "ts"), (v.value for v in dims)))

    def level(self, i, level):
        d = self._level_dims(level)
        img = np.empty((d["h"], d["w"]), np.uint8)
        _check(lib().vs_aligner_read_level_image(self.h, i, level, _p(img)))
        d["img"] = img
        return d

    def keyframe_tables(self, i, level):
        d = self._level_dims(level)
        tx, ty = d["tx"], d["ty"]
        out = {"argmax": [], "jac": []}
        for s in (0, 1):
            am = np.empty((2, ty, tx), np.uint16)
            jc = np.empty((4, ty, tx), np.float32)
            _check(lib().vs_aligner_read_level_argmax(self.h, i, level, s, _p(am)))
            _check(lib().vs_aligner_read_level_jacobian(self.h, i, level, s, _p(jc)))
            out["argmax"].append(am)
            out["jac"].append(jc)
        return out


# ---- the stabilizer --------------------------------------------------------------------------
def stabilizer_params(**kw):
    """StabilizerParams with the library's defaults; a keyword that names a field of the aligner's parameters goes to p.aligner"""
    p = _params(StabilizerParams, "vs_stabilizer_params_default", {})
    _set_fields(p, kw, p.aligner)
    return p


class Stabilizer(_Handle):
    """VideoStabilizer (stabilizer.hpp:32-56) on the GPU engine."""
    _create, _destroy = "vs_stabilizer_create", "vs_stabilizer_destroy"

    def __init__(self, device=0, select_mode=None, border_fill=0, deblur=0, deblur_params=None, denoise=0, denoise_params=None, fill_blend=None,
                 deflicker=0, deflicker_params=None, inpaint=0, rolling_shutter=None, lens=None, scene_cut=None, sharpen=None, output_size=None, **params):
        self.params = stabilizer_params(**params)
        self._open(C.byref(self.params), device)
        if select_mode is not None:
            self.set_select_mode(select_mode)
        if border_fill:
            self.set_border_fill(border_fill)
        if fill_blend:
            self.set_fill_blend(*fill_blend)
        if deblur:
            self.set_deblur(deblur, deblur_params)
        if denoise:
            self.set_denoise(denoise, denoise_params)
        if deflicker:
            self.set_deflicker(deflicker, deflicker_params)
        if inpaint:
            self.set_inpaint(inpaint)
        if rolling_shutter:
            self.set_rolling_shutter(rolling_shutter)
        if lens is not None:
            self.set_lens(*lens)
        if scene_cut is not None:
            self.set_scene_cut(scene_params() if scene_cut is True else scene_cut)
        if sharpen is not None:
            self.set_sharpen(sharpen_params() if sharpen is True else sharpen)
        if output_size is not None:
            self.set_output_size(*output_size)

    def set_output_size(self, dw, dh, filter=RESIZE_LINEAR):
        """(0, 0): off, the crop window is delivered; (-1, -1): every frame is delivered at the source frame's size; (dw, dh): at that size --
        the window resized by THE RESIZE RULE behind every other pass (filter: RESIZE_LINEAR / RESIZE_AREA)"""
        _check(lib().vs_stabilizer_set_output_size(self.h, int(dw), int(dh), int(filter)))

    def get_output_size(self):
        """None (off) or (dw, dh, filter) as set"""
        dw, dh, f = C.c_int(), C.c_int(), C.c_int()
        on = _check(lib().vs_stabilizer_get_output_size(self.h, C.byref(dw), C.byref(dh), C.byref(f)))
        return (dw.value, dh.value, f.value) if on else None

    def delivered_size(self, w, h):
        """(width, height) of what a call with w x h frames delivers: the crop window, or the output size where one is set"""
        c = max(self.params.crop_pixels, 0)
        size = self.get_output_size()
        if size is None:
            return w - 2 * c, h - 2 * c
        return (w, h) if size[0] < 0 else (size[0], size[1])

    def set_sharpen(self, params):
        """None: off; a SharpenParams (sharpen_params()): every output window is sharpened behind the warp by the phase of its own correction
        (VS_WARP_BILINEAR_CV handles)"""
        _check(lib().vs_stabilizer_set_sharpen(self.h, _ref(params)))

    def get_sharpen(self):
        """None (off) or the SharpenParams in force"""
        p = SharpenParams()
        return p if _check(lib().vs_stabilizer_get_sharpen(self.h, C.byref(p))) else None

    def set_scene_cut(self, params):
        """None: off; a SceneParams (scene_params()): every arriving frame is compared with its predecessor through the measured motion, and a
        frame that shows another scene ends every candidate list in front of it and starts a clean path"""
        _check(lib().vs_stabilizer_set_scene_cut(self.h, _ref(params)))

    def get_scene_cut(self):
        """None (off) or the SceneParams in force"""
        p = SceneParams()
        return p if _check(lib().vs_stabilizer_get_scene_cut(self.h, C.byref(p))) else None

    def scene_cuts(self, cap=256):
        """(the number of cuts since the last reset, the 0-based indices since that reset of the most recent min(total, cap, 256) cut frames)"""
        buf = (C.c_int64 * max(cap, 1))()
        total = _check(lib().vs_stabilizer_get_scene_cuts(self.h, buf, int(cap)))
        return total, [int(buf[k]) for k in range(min(total, cap, 256))]

    def set_lens(self, params, w=0, h=0):
        """None (or the identity lens): off; else every arriving w x h frame is remapped through the lens map of `params` (LensParams) in front of
        everything: the aligner and every pass see corrected frames"""
        _check(lib().vs_stabilizer_set_lens(self.h, _ref(params), int(w), int(h)))

    def get_lens(self):
        """None (off) or (LensParams, w, h)"""
        p, w, h = LensParams(), C.c_int(), C.c_int()
        on = _check(lib().vs_stabilizer_get_lens(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return (p, w.value, h.value) if on else None

    def set_rolling_shutter(self, readout):
        """None or 0: off; else every frame is corrected for a rolling shutter of that readout share (-1 .. 1) by the motion to the next input
        frame, before it is warped"""
        _check(lib().vs_stabilizer_set_rolling_shutter(self.h, _ref(RollingParams(float(readout)) if readout is not None else None)))

    def get_rolling_shutter(self):
        p = RollingParams()
        _check(lib().vs_stabilizer_get_rolling_shutter(self.h, C.byref(p)))
        return p.readout

    def set_inpaint(self, on=1):
        """0: off; 1: what neither the frame nor a fill candidate covers in the output window is inpainted (VS_WARP_BILINEAR_CV handles)"""
        _check(lib().vs_stabilizer_set_inpaint(self.h, int(on)))

    def get_inpaint(self):
        return _check(lib().vs_stabilizer_get_inpaint(self.h))

    def set_deflicker(self, ahead, params=None):
        """0: off; 1 .. lag: every output frame's exposure is pulled to the mean exposure of itself and the next `ahead` input frames
        (params: DeflickerParams, None = defaults)"""
        _check(lib().vs_stabilizer_set_deflicker(self.h, int(ahead), _ref(params)))

    def get_deflicker(self):
        return _check(lib().vs_stabilizer_get_deflicker(self.h))

    def set_denoise(self, ahead, params=None):
        """0: off; 1 .. lag: every frame is averaged with what the next `ahead` input frames show at the same scene point before it is warped
        (params: DenoiseParams, None = defaults)"""
        _check(lib().vs_stabilizer_set_denoise(self.h, int(ahead), _ref(params)))

    def get_denoise(self):
        return _check(lib().vs_stabilizer_get_denoise(self.h))

    def set_deblur(self, ahead, params=None):
        """0: off; 1 .. lag: every frame is deblurred from the next `ahead` input frames before it is warped (params: DeblurParams, None = defaults)"""
        _check(lib().vs_stabilizer_set_deblur(self.h, int(ahead), _ref(params)))

    def deblur(self):
        return _check(lib().vs_stabilizer_get_deblur(self.h))

    def set_border_fill(self, ahead):
        """0: off; 1 .. lag: what the corrected frame does not cover is filled from the next `ahead` input frames (VS_WARP_BILINEAR_CV handles)"""
        _check(lib().vs_stabilizer_set_border_fill(self.h, int(ahead)))

    def border_fill(self):
        return _check(lib().vs_stabilizer_get_border_fill(self.h))

    def set_fill_blend(self, feather=0, match=0):
        """the border fill's seam blend: feather 0 (off) or 1 .. 6, match 0 / 1 (exposure match); (0, 0): off (VS_WARP_BILINEAR_CV handles)"""
        p = FillBlendParams(int(feather), int(match))
        _check(lib().vs_stabilizer_set_fill_blend(self.h, C.byref(p)))

    def fill_blend(self):
        p = FillBlendParams()
        _check(lib().vs_stabilizer_get_fill_blend(self.h, C.byref(p)))
        return p.feather, p.match

    def set_select_mode(self, mode):
        """the selection rule of the stabilizer's aligner (SELECT_DEVICE by default, SELECT_STABLE, SELECT_STL_HOST)"""
        _check(lib().vs_stabilizer_set_select_mode(self.h, mode))

    def select_mode(self):
        return _check(lib().vs_stabilizer_get_select_mode(self.h))

    def process(self, frame, fmt=None):
        frame = np.ascontiguousarray(frame)
        fmt = _fmt_of(frame.dtype, frame.ndim) if fmt is None else fmt
        hh, ww = frame.shape[:2]
        dw, dh = self.delivered_size(ww, hh)
        out = np.empty((dh, dw, 3), frame.dtype)
        ow, oh = C.c_int(), C.c_int()
        r = _check(lib().vs_stabilizer_process(self.h, _p(frame), ww, hh, ww * 3, fmt, MEM_HOST, _p(out), C.byref(ow), C.byref(oh)))
        return out if r == 1 else None

    def reset(self):
        _check(lib().vs_stabilizer_reset(self.h))

    def wait_stream(self, stream_handle):
        _check(lib().vs_stabilizer_wait_stream(self.h, C.c_void_p(stream_handle)))

    def _host_batch(self, frames, fmt, out=None):
        """what the host forms of process_batch / process_clips begin with: frames (n,h,w,3) numpy -> the contiguous frames, n, h, w, the format
        and the destination at the delivered size (`out`, if the caller gave one to reuse)"""
        frames = np.ascontiguousarray(frames)
        n, hh, ww = frames.shape[:3]
        fmt = _fmt_of(frames.dtype, 3) if fmt is None else fmt
        dw, dh = self.delivered_size(ww, hh)
        if out is None:
            out = np.zeros((n, dh, dw, 3), frames.dtype)
        assert out.shape == (n, dh, dw, 3) and out.dtype == frames.dtype and out.flags.c_contiguous
        return frames, n, hh, ww, fmt, out

    def process_batch(self, frames, out=None, fmt=None):
        """frames (n,h,w,3) numpy.  returns (outputs (n,oh,ow,3), has_output list).  out: a buffer of that shape to reuse
        (frames without an output are left untouched in it)"""
        frames, n, hh, ww, fmt, out = self._host_batch(frames, fmt, out)
        has, ow, oh = _batch_outs(n)
        _check(lib().vs_stabilizer_process_batch(self.h, _p(frames), hh * ww * 3, n, ww, hh, ww * 3, fmt, MEM_HOST, _p(out),
                                                 out[0].size, has, C.byref(ow), C.byref(oh)))
        return out, list(has)

    def process_batch_device(self, ptr, n, w, h, fmt, out_ptr):
        """dense device-resident frames in, dense delivered frames out (raw device pointers)"""
        dw, dh = self.delivered_size(w, h)
        has, ow, oh = _batch_outs(n)
        r = _check(lib().vs_stabilizer_process_batch(self.h, _p(ptr), h * w * 3, n, w, h, w * 3, fmt, MEM_DEVICE, _p(out_ptr),
                                                     dh * dw * 3, has, C.byref(ow), C.byref(oh)))
        return r, list(has)

    def process_batch_ycbcr(self, y, cb=None, cr=None, sub=(1, 1), fmt=None, interleaved=None, out_sub=None, out_interleaved="same", out_mono=None,
                            guard=None):
        """the batched form on YCbCr planes in host memory (vs_stabilizer_process_batch_ycbcr): y (n,h,w), cb, cr (n,ch,cw) or None (luma
        only), laid out as in ycbcr_to_bgr_batch.  out_sub / out_interleaved / out_mono: the layout of the output planes (default: the
        input's).  -> ((y, cb, cr) at the output size, has_output list); frames without an output keep `guard` (default 0)"""
        y = np.ascontiguousarray(y)
        n, hh, ww = y.shape
        fmt = _fmt_of(y.dtype, 3) if fmt is None else fmt
        dw, dh = self.delivered_size(ww, hh)
        src = _HostPlanes(n, ww, hh, y.dtype, sub, interleaved, cb is None, None, None, 0)
        src.put(y, cb, cr)
        dst = _HostPlanes(n, dw, dh, y.dtype, sub if out_sub is None else out_sub, interleaved if out_interleaved == "same" else out_interleaved,
                          (cb is None) if out_mono is None else out_mono, None, None, 0 if guard is None else guard)
        has, ow, oh = _batch_outs(n)
        _check(lib().vs_stabilizer_process_batch_ycbcr(self.h, C.byref(src.desc), n, ww, hh, fmt, MEM_HOST, C.byref(dst.desc), has, C.byref(ow), C.byref(oh)))
        assert (ow.value, oh.value) == (dw, dh)
        return dst.get(), list(has)

    def process_batch_ycbcr_device(self, planes, n, w, h, fmt, out_planes):
        """device-resident form: planes / out_planes are YcbcrPlanes of device addresses (ycbcr_planes) -> (outputs, has_output, out_w, out_h)"""
        has, ow, oh = _batch_outs(n)
        r = _check(lib().vs_stabilizer_process_batch_ycbcr(self.h, C.byref(planes), n, w, h, fmt, MEM_DEVICE, C.byref(out_planes), has, C.byref(ow), C.byref(oh)))
        return r, list(has), ow.value, oh.value

    def process_clips(self, frames, n_clips, fmt=None):
        """frames (n_clips*fpc, h, w, 3) numpy: every clip through a fresh stabilizer, batched together"""
        frames, n, hh, ww, fmt, out = self._host_batch(frames, fmt)
        has, ow, oh = _batch_outs(n)
        _check(lib().vs_stabilizer_process_clips(self.h, _p(frames), hh * ww * 3, n_clips, n // n_clips, ww, hh, ww * 3, fmt, MEM_HOST,
                                                 _p(out), out[0].size, has, C.byref(ow), C.byref(oh)))
        return out, list(has)

    def process_clips_device(self, ptr, n_clips, frames_per_clip, w, h, fmt, out_ptr):
        dw, dh = self.delivered_size(w, h)
        n = n_clips * frames_per_clip
        has, ow, oh = _batch_outs(n)
        r = _check(lib().vs_stabilizer_process_clips(self.h, _p(ptr), h * w * 3, n_clips, frames_per_clip, w, h, w * 3, fmt, MEM_DEVICE,
                                                     _p(out_ptr), dh * dw * 3, has, C.byref(ow), C.byref(oh)))
        return r, list(has)

    def state(self):
        m, a, s = Transform(), Transform(), C.c_int()
        lib().vs_stabilizer_state(self.h, C.byref(m), C.byref(a), C.byref(s))
        return m, a, bool(s.value)
