"""codec-eval_amd — MI355X (gfx950) backend for the perceptual-metric hot path of imazen/codec-eval.

The product is ``libce_metrics_hip.so`` (hand-written HIP kernels behind the C ABI declared in
``include/ce_metrics.h``).  This module is the thin ctypes binding used by the tests, bench.py and
Python callers; every metric call goes through the C ABI and there is NO CPU fallback: if the shared
library is missing or no HIP device is visible the call raises.

Import name: the directory is ``codec-eval_amd`` (hyphen, as the repo layout prescribes); use
``import codec_eval_amd`` (the shim module at the repo root) or
``importlib.import_module("codec-eval_amd")``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, replace
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

# HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and a stream that shares a queue with a busy
# one waits for it.  A context uses two streams per batch plus an upload stream, and callers keep several contexts /
# batches in flight, so ask for 16 (read once, when the HIP runtime initialises: this only takes effect if the package
# is imported before the process's first HIP call; 32 is far slower on MI355X, so it is a setdefault, not a maximum).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CE_METRICS_LIB") or os.path.join(_HERE, "libce_metrics_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

# ---- enums of include/ce_metrics.h ---------------------------------------------------------
CE_OK, CE_ERR_DIM_MISMATCH, CE_ERR_BAD_LENGTH, CE_ERR_TOO_SMALL, CE_ERR_BACKEND, CE_ERR_INVALID_ARG = range(6)
METRIC_DSSIM, METRIC_SSIMULACRA2, METRIC_BUTTERAUGLI, METRIC_PSNR = 1, 2, 4, 8
FLAG_XYB_ROUNDTRIP = 1
FLAG_BUTTERAUGLI_DIFFMAP = 1 << 1
FLAG_SSIMULACRA2_MAPS = 1 << 2
PIXEL_RGB8, PIXEL_RGBA8, PIXEL_RGB16_10BIT, PIXEL_RGBA16_10BIT = 0, 1, 2, 3
PIXEL_RGB16, PIXEL_RGBA16 = 4, 5  # deep batches only (Context.batch_deep): u16 samples at the side's own depth
PIXEL_RGB_F32 = 7  # linear batches only (Context.batch_linear): packed float RGB, linear light with sRGB primaries
PIXEL_RGBA_F32 = 8  # packed float RGBA, linear light: Batch.set_*_linear_over and Context.linear_over only
LINEAR_MAX = 1024.0  # CE_LINEAR_MAX: the clamp of a linear image's samples on ingest
DEEP_DEPTHS = (8, 10, 12, 16)
# ITU-T H.273 code points the CICP ingest takes (include/ce_metrics.h)
PRIMARIES_BT709, PRIMARIES_BT2020, PRIMARIES_P3_D65 = 1, 9, 12
TRANSFER_SRGB, TRANSFER_LINEAR, TRANSFER_PQ = 13, 8, 16
TRANSFER_HLG = 18  # not a ce_colour transfer: HLG carries a display description of its own (HlgDescription)
BATCH_REFERENCES, BATCH_TESTS = 0, 1  # enum ce_batch_images
DEFAULT_INTENSITY_TARGET = 80.0
DSSIM_MAX_LEVELS = 5  # CE_DSSIM_MAX_LEVELS
SSIM2_MAX_SCALES = 6  # CE_SSIM2_MAX_SCALES
SSIM2_MAP_SSIM, SSIM2_MAP_ARTIFACT, SSIM2_MAP_DETAIL_LOST = 0, 1, 2  # enum ce_ssim2_map
RESAMPLE_BOX, RESAMPLE_BILINEAR, RESAMPLE_BICUBIC, RESAMPLE_LANCZOS3 = 0, 1, 2, 3  # enum ce_resample_filter
# planar Y'CbCr ingest (include/ce_metrics.h)
YUV_444, YUV_422, YUV_420, YUV_400 = 0, 1, 2, 3  # enum ce_yuv_subsampling
YUV_PLANAR, YUV_SEMIPLANAR = 0, 1  # enum ce_yuv_layout
YUV_BT601, YUV_BT709, YUV_BT2020 = 0, 1, 2  # enum ce_yuv_matrix
YUV_FULL, YUV_LIMITED = 0, 1  # enum ce_yuv_range
CHROMA_NEAREST, CHROMA_TRIANGLE = 0, 1  # enum ce_chroma_upsample
MEM_HOST, MEM_DEVICE = 0, 1  # enum ce_mem
# tensor ingest (include/ce_metrics.h)
DTYPE_U8, DTYPE_U16, DTYPE_F16, DTYPE_BF16, DTYPE_F32 = 0, 1, 2, 3, 4  # enum ce_dtype
QUANT_NEAREST_EVEN, QUANT_TRUNCATE = 0, 1  # enum ce_quantise
MAX_BACKGROUNDS = 8  # CE_MAX_BACKGROUNDS: solid colours one upload is composited over
ALPHA_BLACK_WHITE = ((0, 0, 0), (255, 255, 255))  # the two page colours a transparent image is most often seen on, 8-bit
# EvalConfig.alpha_blend: transparent images scored in linear light are blended over alpha_backgrounds THERE, after the pixel
# has been turned into linear light (Batch.set_*_cicp_over and its kin)
ALPHA_BLEND_LINEAR = "linear"

_STATUS_NAMES = {
    CE_ERR_DIM_MISMATCH: "DimensionMismatch",
    CE_ERR_BAD_LENGTH: "MetricCalculation(invalid image size)",
    CE_ERR_TOO_SMALL: "MetricCalculation(image too small)",
    CE_ERR_BACKEND: "MetricCalculation(backend)",
    CE_ERR_INVALID_ARG: "InvalidArgument",
}


class CeScores(C.Structure):
    _fields_ = [
        ("dssim", C.c_double),
        ("ssimulacra2", C.c_double),
        ("butteraugli", C.c_double),
        ("psnr", C.c_double),
        ("valid", C.c_uint32),
        ("status", C.c_int32),
    ]


class CePairDesc(C.Structure):
    _fields_ = [
        ("reference", C.c_void_p),
        ("reference_len", C.c_size_t),
        ("test", C.c_void_p),
        ("test_len", C.c_size_t),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
    ]


# ImageHeuristics of crates/codec-compare/src/image_heuristics.rs:22-63 without the name, plus analyze-image's
# "variance > 1000" block percentage (analyze_image.rs:94-96): the fields of ce_image_heuristics, in order
HEURISTICS_FIELDS = (
    "width", "height", "pixels",
    "mean_luminance", "luminance_variance", "luminance_std",
    "edge_strength_mean", "edge_strength_max", "edge_density",
    "flat_block_pct", "low_var_block_pct", "mid_var_block_pct", "high_var_block_pct", "detail_block_pct",
    "block_variance_mean", "block_variance_std",
    "color_variance", "saturation_mean", "saturation_std",
    "high_freq_energy", "low_freq_energy", "freq_ratio",
    "local_contrast_mean", "local_contrast_std",
    "horizontal_complexity", "vertical_complexity", "diagonal_complexity",
    "analyze_detail_block_pct",
)


class CeImageHeuristics(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in HEURISTICS_FIELDS[:3]] + [(f, C.c_float) for f in HEURISTICS_FIELDS[3:]]


class CeYuvImage(C.Structure):
    _fields_ = [
        ("plane", C.c_void_p * 3),
        ("pitch", C.c_size_t * 3),
        ("subsampling", C.c_int),
        ("layout", C.c_int),
        ("matrix", C.c_int),
        ("range", C.c_int),
        ("upsample", C.c_int),
        ("depth", C.c_int),
        ("msb_aligned", C.c_int),
        ("memory", C.c_int),
        ("lut", C.c_void_p),
    ]


class CeTensorImage(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("stride_n", C.c_int64),
        ("stride_c", C.c_int64),
        ("stride_y", C.c_int64),
        ("stride_x", C.c_int64),
        ("dtype", C.c_int),
        ("memory", C.c_int),
        ("quantise", C.c_int),
    ]


class CeColour(C.Structure):
    _fields_ = [("primaries", C.c_int), ("transfer", C.c_int), ("depth", C.c_uint32), ("white_nits", C.c_float)]


class CeHlg(C.Structure):
    _fields_ = [("primaries", C.c_int), ("depth", C.c_uint32), ("peak_nits", C.c_float), ("system_gamma", C.c_float), ("white_nits", C.c_float)]


class CeGainmapImage(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32)]


class CeGainmap(C.Structure):
    _fields_ = [("gain_min", C.c_float * 3), ("gain_max", C.c_float * 3), ("gamma", C.c_float * 3), ("base_offset", C.c_float * 3),
                ("alternate_offset", C.c_float * 3), ("base_headroom", C.c_float), ("alternate_headroom", C.c_float),
                ("display_headroom", C.c_float)]


class CeIccCurve(C.Structure):
    _fields_ = [("type", C.c_int), ("count", C.c_uint32), ("params", C.c_int32 * 7), ("offset", C.c_uint32)]


class CeIccDescription(C.Structure):
    _fields_ = [("kind", C.c_int), ("version", C.c_uint32), ("profile_class", C.c_uint32), ("colorants", C.c_int32 * 9),
                ("curves", CeIccCurve * 3), ("reason", C.c_char * 96)]


class CeIccLutDescription(C.Structure):
    _fields_ = [("kind", C.c_int), ("version", C.c_uint32), ("profile_class", C.c_uint32), ("pcs", C.c_uint32), ("tag", C.c_uint32),
                ("tag_type", C.c_uint32), ("tag_offset", C.c_uint32), ("tag_size", C.c_uint32), ("stages", C.c_uint32), ("grid", C.c_uint32 * 3),
                ("precision", C.c_uint32), ("clut_offset", C.c_uint32), ("matrix", C.c_int32 * 12), ("a", CeIccCurve * 3), ("m", CeIccCurve * 3),
                ("b", CeIccCurve * 3), ("reason", C.c_char * 96)]


class CeIccLutCurve(C.Structure):
    _fields_ = [("kind", C.c_int), ("ftype", C.c_uint32), ("count", C.c_uint32), ("first_sample", C.c_uint32), ("q", C.c_double * 7)]


class CeHdrScores(C.Structure):
    _fields_ = [("pq_psnr", C.c_double), ("delta_e_itp_mean", C.c_double), ("delta_e_itp_max", C.c_double),
                ("pq_sse", C.c_uint64), ("itp_sum_q20", C.c_uint64), ("itp_max_q20", C.c_uint64)]


class CeMsssimScores(C.Structure):
    _fields_ = [("ms_ssim", C.c_double), ("ssim", C.c_double), ("ms_ssim_rgb", C.c_double * 3), ("ssim_rgb", C.c_double * 3),
                ("ssim_q", (C.c_int64 * 3) * 5), ("cs_q", (C.c_int64 * 3) * 5), ("n", C.c_uint64 * 5), ("n_levels", C.c_uint32),
                ("reserved", C.c_uint32)]


class CeCiede2000Scores(C.Structure):
    _fields_ = [("sum_q20", C.c_uint64), ("n", C.c_uint64), ("n_above", C.c_uint64 * 8), ("mean", C.c_double), ("max", C.c_double),
                ("ciede2000_db", C.c_double), ("max_q20", C.c_uint32), ("n_thresholds", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CePlaneScores(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("n", C.c_uint64 * 3), ("psnr", C.c_double * 3), ("psnr_weighted", C.c_double),
                ("psnr_overall", C.c_double), ("ssim", C.c_double * 3), ("ms_ssim", C.c_double * 3), ("ssim_q", (C.c_int64 * 5) * 3),
                ("cs_q", (C.c_int64 * 5) * 3), ("n_pos", (C.c_uint64 * 5) * 3), ("n_levels", C.c_uint32 * 3), ("n_planes", C.c_uint32)]


class CePlaneHvsScores(C.Structure):
    _fields_ = [("hvs_q", (C.c_uint64 * 2) * 3), ("hvsm_q", (C.c_uint64 * 2) * 3), ("n_blocks", C.c_uint64 * 3),
                ("psnr_hvs", C.c_double * 3), ("psnr_hvsm", C.c_double * 3), ("n_planes", C.c_uint32), ("step", C.c_uint32)]


class CePlaneVifScores(C.Structure):
    _fields_ = [("num_q", (C.c_uint64 * 4) * 3), ("den_q", (C.c_uint64 * 4) * 3), ("n_pos", (C.c_uint64 * 4) * 3),
                ("vif_scale", (C.c_double * 4) * 3), ("vifp", C.c_double * 3), ("ran", C.c_uint32 * 3), ("n_planes", C.c_uint32)]


class CePlaneGmsdScores(C.Structure):
    _fields_ = [("sum_q", C.c_uint64 * 3), ("sum_q2", (C.c_uint64 * 2) * 3), ("n_pos", C.c_uint64 * 3), ("gmsd", C.c_double * 3),
                ("gmsm", C.c_double * 3), ("max_dis", C.c_uint32 * 3), ("n_planes", C.c_uint32)]


class CodecEvalError(RuntimeError):
    """Mirrors codec_eval::Error for this path (src/error.rs:31-49)."""

    def __init__(self, status: int, message: str = ""):
        self.status = status
        self.kind = _STATUS_NAMES.get(status, f"status {status}")
        super().__init__(f"{self.kind}: {message}" if message else self.kind)


class DimensionMismatch(CodecEvalError):
    pass


class MetricCalculation(CodecEvalError):
    pass


def _raise(status: int, message: str):
    if status == CE_ERR_DIM_MISMATCH:
        raise DimensionMismatch(status, message)
    if status in (CE_ERR_BAD_LENGTH, CE_ERR_TOO_SMALL, CE_ERR_BACKEND):
        raise MetricCalculation(status, message)
    raise CodecEvalError(status, message)


def _error_obj(status: int, message: str) -> CodecEvalError:
    try:
        _raise(status, message)
    except CodecEvalError as e:
        return e


_lib: Optional[C.CDLL] = None

# (name, restype, argtypes) — must list every function include/ce_metrics.h declares
_vp, _u8p, _sz, _u32, _f32, _i = C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_float, C.c_int
_dp = C.POINTER(C.c_double)
_PROTOTYPES = [
    ("ce_version", C.c_char_p, []),
    ("ce_device_count", _i, []),
    ("ce_ctx_create", _i, [_i, C.POINTER(_vp)]),
    ("ce_ctx_create_on_stream", _i, [_i, _vp, C.POINTER(_vp)]),
    ("ce_ctx_destroy", None, [_vp]),
    ("ce_ctx_synchronize", _i, [_vp]),
    ("ce_ctx_stream", _vp, [_vp]),
    ("ce_last_error", C.c_char_p, [_vp]),
    ("ce_calculate_psnr", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _dp]),
    ("ce_calculate_ssimulacra2", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _dp]),
    ("ce_calculate_dssim", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _dp]),
    ("ce_calculate_butteraugli", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _f32, _dp]),
    ("ce_calculate_butteraugli_diffmap", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _f32, _dp, _vp]),
    ("ce_dssim_levels", _i, [_u32, _u32, C.POINTER(_u32), _vp, _vp]),
    ("ce_calculate_dssim_ssim_maps", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _dp, _vp, _vp, _sz]),
    ("ce_ssimulacra2_scales", _i, [_u32, _u32, C.POINTER(_u32), _vp, _vp]),
    ("ce_calculate_ssimulacra2_maps", _i, [_vp, _u8p, _sz, _u8p, _sz, _sz, _sz, _dp, _vp, _vp, _sz]),
    ("ce_xyb_roundtrip", _i, [_vp, _u8p, _sz, _sz, _sz, _u8p]),
    ("ce_rgb8_to_dssim_image", _i, [_vp, _u8p, _sz, _sz, _sz, _vp]),
    ("ce_eval_pair", _i, [_vp, _u8p, _sz, _u8p, _sz, _u32, _u32, _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_eval_batch", _i, [_vp, _sz, C.POINTER(CePairDesc), _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_estimate_batch_bytes", _sz, [_u32, _u32, _u32, _u32, _u32]),
    ("ce_ctx_memory_info", _i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    ("ce_host_alloc", _i, [_vp, _sz, C.POINTER(_vp)]),
    ("ce_host_free", _i, [_vp, _vp]),
    ("ce_eval_batch_lut", _i, [_vp, _sz, C.POINTER(CePairDesc), C.POINTER(_vp), _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_batch_create", _i, [_vp, _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    ("ce_batch_destroy", None, [_vp]),
    ("ce_pixel_bytes", _sz, [_i]),
    ("ce_batch_create_deep", _i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    ("ce_estimate_batch_bytes_deep", _sz, [_u32, _u32, _u32, _u32, _u32, _u32, _u32]),
    ("ce_eval_pair_deep", _i, [_vp, _vp, _sz, _u32, _vp, _sz, _u32, _u32, _u32, _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_batch_create_linear", _i, [_vp, _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    ("ce_estimate_batch_bytes_linear", _sz, [_u32, _u32, _u32, _u32, _u32]),
    ("ce_eval_pair_linear", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_srgb_table", _i, [_u32, _i, _vp, _sz]),
    ("ce_batch_set_reference_cicp", _i, [_vp, _u32, _vp, _sz, _i, C.POINTER(CeColour)]),
    ("ce_batch_set_test_cicp", _i, [_vp, _u32, _u32, _vp, _sz, _i, C.POINTER(CeColour)]),
    ("ce_cicp_to_linear", _i, [_vp, _vp, _sz, _i, C.POINTER(CeColour), _u32, _u32, _vp, _sz]),
    ("ce_transfer_table", _i, [_i, _u32, _f32, _vp, _sz]),
    ("ce_colour_matrix", _i, [_i, _vp]),
    ("ce_batch_set_reference", _i, [_vp, _u32, _u8p, _sz]),
    ("ce_batch_set_test", _i, [_vp, _u32, _u32, _u8p, _sz]),
    ("ce_batch_set_reference_fmt", _i, [_vp, _u32, _vp, _sz, _i]),
    ("ce_batch_set_test_fmt", _i, [_vp, _u32, _u32, _vp, _sz, _i]),
    ("ce_lut_create", _i, [_vp, _u8p, _sz, C.POINTER(_vp)]),
    ("ce_lut_destroy", None, [_vp]),
    ("ce_batch_set_reference_lut", _i, [_vp, _u32, _vp, _sz, _i, _vp]),
    ("ce_batch_set_test_lut", _i, [_vp, _u32, _u32, _vp, _sz, _i, _vp]),
    ("ce_batch_reference_slab", _vp, [_vp]),
    ("ce_batch_references_changed", _i, [_vp]),
    ("ce_batch_ref_stats", _i, [_vp, C.POINTER(_u32 * 3)]),
    ("ce_batch_test_slab", _vp, [_vp]),
    ("ce_batch_bind_pair", _i, [_vp, _u32, _u32]),
    ("ce_batch_run", _i, [_vp, _u32, _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_batch_launch", _i, [_vp, _u32, _u32, _u32, _f32]),
    ("ce_batch_collect", _i, [_vp, _u32, C.POINTER(CeScores)]),
    ("ce_batch_butteraugli_pnorm3", _i, [_vp, _u32, _dp]),
    ("ce_batch_butteraugli_diffmap", _i, [_vp, _u32, _u32, _u32, _vp, _sz]),
    ("ce_batch_dssim_ssim_maps", _i, [_vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    ("ce_batch_ssimulacra2_maps", _i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    ("ce_ref_create", _i, [_vp, _u8p, _sz, _u32, _u32, _u32, C.POINTER(_vp)]),
    ("ce_ref_compare", _i, [_vp, _u8p, _sz, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_ref_compare_many", _i, [_vp, C.POINTER(_u8p), C.POINTER(_sz), _u32, _u32, _f32, C.POINTER(CeScores)]),
    ("ce_ref_stats", _i, [_vp, C.POINTER(_u32 * 3)]),
    ("ce_ref_butteraugli_diffmap", _i, [_vp, _u32, _u32, _u32, _vp, _sz]),
    ("ce_ref_dssim_ssim_maps", _i, [_vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    ("ce_ref_ssimulacra2_maps", _i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    ("ce_ref_destroy", None, [_vp]),
    ("ce_image_heuristics_rgb8", _i, [_vp, _u8p, _sz, _sz, _sz, C.POINTER(CeImageHeuristics)]),
    ("ce_batch_image_heuristics", _i, [_vp, _u32, _u32, _u32, C.POINTER(CeImageHeuristics)]),
    ("ce_ref_image_heuristics", _i, [_vp, C.POINTER(CeImageHeuristics)]),
    ("ce_resample_rgb8", _i, [_vp, _u8p, _sz, _u32, _u32, _u32, _u32, _i, _u8p, _sz]),
    ("ce_resample_linear", _i, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _i, _vp, _sz]),
    ("ce_batch_resample", _i, [_vp, _vp, _u32, _u32, _u32, _i]),
    ("ce_batch_resample_pairs", _i, [_vp, _vp, _u32, _u32, _i]),
    ("ce_yuv_coefficients", _i, [_i, _i, _u32, _u32, C.POINTER(C.c_int64 * 7)]),
    ("ce_batch_set_reference_yuv", _i, [_vp, _u32, C.POINTER(CeYuvImage)]),
    ("ce_batch_set_test_yuv", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage)]),
    ("ce_yuv_to_rgb8", _i, [_vp, C.POINTER(CeYuvImage), _u32, _u32, _vp, _sz]),
    ("ce_yuv_to_rgb16", _i, [_vp, C.POINTER(CeYuvImage), _u32, _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_yuv_cicp", _i, [_vp, _u32, C.POINTER(CeYuvImage), C.POINTER(CeColour)]),
    ("ce_batch_set_test_yuv_cicp", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), C.POINTER(CeColour)]),
    ("ce_yuv_to_linear", _i, [_vp, C.POINTER(CeYuvImage), C.POINTER(CeColour), _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_yuv_icc", _i, [_vp, _u32, C.POINTER(CeYuvImage), _u32, _vp]),
    ("ce_batch_set_test_yuv_icc", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), _u32, _vp]),
    ("ce_yuv_icc_to_linear", _i, [_vp, C.POINTER(CeYuvImage), _u32, _vp, _u32, _u32, _vp, _sz]),
    ("ce_yuv_icc_to_srgb8", _i, [_vp, C.POINTER(CeYuvImage), _u32, _vp, _u32, _u32, _vp, _sz]),
    ("ce_yuv_icc_to_srgb16", _i, [_vp, C.POINTER(CeYuvImage), _u32, _vp, _u32, _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_hlg", _i, [_vp, _u32, _vp, _sz, _i, C.POINTER(CeHlg)]),
    ("ce_batch_set_test_hlg", _i, [_vp, _u32, _u32, _vp, _sz, _i, C.POINTER(CeHlg)]),
    ("ce_hlg_to_linear", _i, [_vp, _vp, _sz, _i, C.POINTER(CeHlg), _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_yuv_hlg", _i, [_vp, _u32, C.POINTER(CeYuvImage), C.POINTER(CeHlg)]),
    ("ce_batch_set_test_yuv_hlg", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), C.POINTER(CeHlg)]),
    ("ce_yuv_hlg_to_linear", _i, [_vp, C.POINTER(CeYuvImage), C.POINTER(CeHlg), _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_tensor", _i, [_vp, _u32, _u32, C.POINTER(CeTensorImage)]),
    ("ce_batch_set_test_tensor", _i, [_vp, _u32, _vp, _u32, C.POINTER(CeTensorImage)]),
    ("ce_tensor_to_rgb8", _i, [_vp, C.POINTER(CeTensorImage), _u32, _u32, _vp, _sz]),
    ("ce_tensor_to_rgb16", _i, [_vp, C.POINTER(CeTensorImage), _u32, _u32, _u32, _vp, _sz]),
    ("ce_tensor_to_linear", _i, [_vp, C.POINTER(CeTensorImage), _u32, _u32, _vp, _sz]),
    ("ce_hlg_table", _i, [_u32, _vp, _sz]),
    ("ce_hlg_params", _i, [C.POINTER(CeHlg), _dp]),
    ("ce_batch_set_reference_gainmap", _i, [_vp, _u32, _vp, _sz, _i, C.POINTER(CeColour), C.POINTER(CeGainmapImage), C.POINTER(CeGainmap)]),
    ("ce_batch_set_test_gainmap", _i, [_vp, _u32, _u32, _vp, _sz, _i, C.POINTER(CeColour), C.POINTER(CeGainmapImage), C.POINTER(CeGainmap)]),
    ("ce_gainmap_to_linear", _i, [_vp, _vp, _sz, _i, C.POINTER(CeColour), C.POINTER(CeGainmapImage), C.POINTER(CeGainmap), _u32, _u32, _vp, _sz]),
    ("ce_gainmap_tables", _i, [C.POINTER(CeGainmap), _u32, _dp, _sz]),
    ("ce_gainmap_weight", _i, [C.POINTER(CeGainmap), _dp]),
    ("ce_batch_hdr_fidelity", _i, [_vp, _u32, _u32, _f32, C.POINTER(CeHdrScores)]),
    ("ce_eval_pair_hdr_fidelity", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _f32, C.POINTER(CeHdrScores)]),
    ("ce_pq_code_thresholds", _i, [_u32, _f32, _vp, _sz]),
    ("ce_hdr_fidelity_matrices", _i, [_vp, _vp]),
    ("ce_batch_delta_e_itp_map", _i, [_vp, _u32, _u32, _u32, _f32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_eval_pair_delta_e_itp_map", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _f32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_batch_msssim", _i, [_vp, _u32, _u32, C.POINTER(CeMsssimScores)]),
    ("ce_eval_pair_msssim", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, C.POINTER(CeMsssimScores)]),
    ("ce_eval_pair_msssim_deep", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, C.POINTER(CeMsssimScores)]),
    ("ce_yuv_plane_fidelity", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), _u32, C.POINTER(CeYuvImage), _u32, _vp, _u32,
                               C.POINTER(CePlaneScores)]),
    ("ce_yuv_plane_hvs", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), _u32, C.POINTER(CeYuvImage), _u32, _vp, _u32,
                          C.POINTER(CePlaneHvsScores)]),
    ("ce_yuv_plane_vif", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), _u32, C.POINTER(CeYuvImage), _u32, _vp, C.POINTER(CePlaneVifScores)]),
    ("ce_vif_window", _i, [_u32, _vp]),
    ("ce_yuv_plane_gmsd", _i, [_vp, _u32, _u32, C.POINTER(CeYuvImage), _u32, C.POINTER(CeYuvImage), _u32, _vp, C.POINTER(CePlaneGmsdScores)]),
    ("ce_batch_msssim_map", _i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_eval_pair_msssim_map", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_eval_pair_msssim_map_deep", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_msssim_window", _i, [_vp]),
    ("ce_batch_ciede2000", _i, [_vp, _u32, _vp, _u32, C.POINTER(CeCiede2000Scores)]),
    ("ce_eval_pair_ciede2000", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _vp, _u32, C.POINTER(CeCiede2000Scores)]),
    ("ce_eval_pair_ciede2000_deep", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _vp, _u32, C.POINTER(CeCiede2000Scores)]),
    ("ce_ciede2000_pixels", _i, [_vp, _u32, _vp, _u32, _sz, _vp]),
    ("ce_batch_ciede2000_map", _i, [_vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_eval_pair_ciede2000_map", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_eval_pair_ciede2000_map_deep", _i, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _u32, _vp]),
    ("ce_ciede2000_pixel_terms", _i, [_vp, _u32, _vp, _u32, _sz, _vp]),
    ("ce_msssim_levels", _i, [_u32, _u32, _u32, _vp, _vp, _vp]),
    ("ce_icc_describe", _i, [_vp, _sz, C.POINTER(CeIccDescription)]),
    ("ce_icc_build_matrix", _i, [_vp, _sz, _vp]),
    ("ce_icc_build_tables", _i, [_vp, _sz, _u32, _vp, _sz]),
    ("ce_srgb_encode_thresholds", _i, [_u32, _vp, _sz]),
    ("ce_icc_create", _i, [_vp, _vp, _sz, C.POINTER(_vp)]),
    ("ce_icc_lut_describe", _i, [_vp, _sz, _i, C.POINTER(CeIccLutDescription)]),
    ("ce_icc_lut_build_input_tables", _i, [_vp, _sz, _i, _u32, _vp, _sz]),
    ("ce_icc_lut_build_clut", _i, [_vp, _sz, _i, _vp, _sz]),
    ("ce_icc_lut_build_matrix", _i, [_vp, _sz, _i, _vp]),
    ("ce_icc_lut_build_curves", _i, [_vp, _sz, _i, C.POINTER(CeIccLutCurve), _vp, _sz, C.POINTER(C.c_size_t)]),
    ("ce_icc_lut_build_pcs_matrix", _i, [_vp]),
    ("ce_icc_lut_create", _i, [_vp, _vp, _sz, _i, _i, C.POINTER(_vp)]),
    ("ce_icc_destroy", None, [_vp]),
    ("ce_batch_set_reference_icc", _i, [_vp, _u32, _vp, _sz, _i, _u32, _vp]),
    ("ce_batch_set_test_icc", _i, [_vp, _u32, _u32, _vp, _sz, _i, _u32, _vp]),
    ("ce_icc_to_linear", _i, [_vp, _vp, _sz, _i, _u32, _vp, _u32, _u32, _vp, _sz]),
    ("ce_icc_to_srgb8", _i, [_vp, _vp, _sz, _i, _u32, _vp, _u32, _u32, _vp, _sz]),
    ("ce_icc_to_srgb16", _i, [_vp, _vp, _sz, _i, _u32, _vp, _u32, _u32, _u32, _vp, _sz]),
    ("ce_batch_set_reference_over", _i, [_vp, _u32, _vp, _sz, _i, _u32, _vp]),
    ("ce_batch_set_test_over", _i, [_vp, _u32, _vp, _vp, _sz, _i, _u32, _vp]),
    ("ce_composite_rgba8", _i, [_vp, _vp, _sz, _u32, _u32, _vp, _vp, _sz]),
    ("ce_alpha_table", _i, [_u32, _vp, _sz]),
    ("ce_batch_set_reference_cicp_over", _i, [_vp, _u32, _vp, _sz, _i, C.POINTER(CeColour), _u32, _vp]),
    ("ce_batch_set_test_cicp_over", _i, [_vp, _u32, _vp, _vp, _sz, _i, C.POINTER(CeColour), _u32, _vp]),
    ("ce_batch_set_reference_hlg_over", _i, [_vp, _u32, _vp, _sz, _i, C.POINTER(CeHlg), _u32, _vp]),
    ("ce_batch_set_test_hlg_over", _i, [_vp, _u32, _vp, _vp, _sz, _i, C.POINTER(CeHlg), _u32, _vp]),
    ("ce_batch_set_reference_icc_over", _i, [_vp, _u32, _vp, _sz, _i, _u32, _vp, _u32, _vp]),
    ("ce_batch_set_test_icc_over", _i, [_vp, _u32, _vp, _vp, _sz, _i, _u32, _vp, _u32, _vp]),
    ("ce_batch_set_reference_linear_over", _i, [_vp, _u32, _vp, _sz, _i, _i, _u32, _vp]),
    ("ce_batch_set_test_linear_over", _i, [_vp, _u32, _vp, _vp, _sz, _i, _i, _u32, _vp]),
    ("ce_cicp_over_to_linear", _i, [_vp, _vp, _sz, _i, C.POINTER(CeColour), _u32, _u32, _vp, _vp, _sz]),
    ("ce_hlg_over_to_linear", _i, [_vp, _vp, _sz, _i, C.POINTER(CeHlg), _u32, _u32, _vp, _vp, _sz]),
    ("ce_icc_over_to_linear", _i, [_vp, _vp, _sz, _i, _u32, _vp, _u32, _u32, _vp, _vp, _sz]),
    ("ce_linear_over", _i, [_vp, _vp, _sz, _i, _i, _u32, _u32, _vp, _vp, _sz]),
    ("ce_composite_rgba16", _i, [_vp, _vp, _sz, _u32, _u32, _u32, _vp, _vp, _sz]),
    ("ce_prof_enable", _i, [_vp, _i]),
    ("ce_prof_filter", _i, [_vp, C.c_char_p]),
    ("ce_prof_reset", _i, [_vp]),
    ("ce_prof_count", _i, [_vp]),
    ("ce_prof_get", _i, [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), _dp]),
    ("ce_timer_start", _i, [_vp]),
    ("ce_timer_stop", _i, [_vp, _dp]),
    ("ce_debug_ssim2_planes", _i, [_vp, _i, _i, _i, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    ("ce_debug_ssim2_limit_scales", _i, [_vp, _i]),
    ("ce_debug_ssim2_averages", _i, [_vp, _u32, _dp, C.POINTER(_i)]),
    ("ce_debug_ssim2_occupancy", _i, [_i]),
    ("ce_debug_cbrt_sweep", _i, [_vp, _u32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("ce_debug_div_sweep", _i, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("ce_debug_calibrate_traffic", _i, [_vp, _sz]),
    ("ce_debug_dssim_walk_rows", _i, [_vp, _u32]),
]
ABI_SYMBOLS = [p[0] for p in _PROTOTYPES]


def lib() -> C.CDLL:
    """Load libce_metrics_hip.so (built by __graft_entry__.build() / codec-eval_amd/build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback."
            )
        _lib = C.CDLL(LIB_PATH)
        for name, restype, argtypes in _PROTOTYPES:
            fn = getattr(_lib, name)  # AttributeError here = ABI symbol missing
            fn.restype = restype
            fn.argtypes = argtypes
    return _lib


def estimate_batch_bytes(width: int, height: int, n_refs: int, n_pairs: int, config: "MetricConfig") -> int:
    """Upper estimate of the device bytes a Batch of this shape holds once `config`'s metrics have run."""
    return int(lib().ce_estimate_batch_bytes(width, height, n_refs, n_pairs, config.mask))


def estimate_batch_bytes_deep(width: int, height: int, n_refs: int, n_pairs: int, config: "MetricConfig", ref_depth: int,
                              test_depth: int) -> int:
    """estimate_batch_bytes for a deep batch (Context.batch_deep) of these depths."""
    return int(lib().ce_estimate_batch_bytes_deep(width, height, n_refs, n_pairs, config.mask, ref_depth, test_depth))


def estimate_batch_bytes_linear(width: int, height: int, n_refs: int, n_pairs: int, config: "MetricConfig") -> int:
    """estimate_batch_bytes for a linear batch (Context.batch_linear)."""
    return int(lib().ce_estimate_batch_bytes_linear(width, height, n_refs, n_pairs, config.mask))


def _host_check(rc: int):
    if rc != CE_OK:
        _raise(rc, (lib().ce_last_error(None) or b"").decode())


def srgb_table(depth: int, rule: int = 0) -> np.ndarray:
    """The library's own sRGB -> linear table of `depth` bits (ce_srgb_table): rule 0 the f64 curve rounded once to f32
    (SSIMULACRA2, Butteraugli), rule 1 f32 powf (DSSIM) - exactly the floats the RGB8 and deep batches read."""
    out = np.empty(1 << depth if 0 < depth <= 16 else 1, np.float32)
    _host_check(lib().ce_srgb_table(depth, rule, out.ctypes.data, out.size))
    return out


def transfer_table(transfer: int, depth: int, white_nits: float = 203.0) -> np.ndarray:
    """The CICP ingest's table of code value -> linear light (ce_transfer_table); white_nits is read for PQ only."""
    out = np.empty(1 << depth if 0 < depth <= 16 else 1, np.float32)
    _host_check(lib().ce_transfer_table(transfer, depth, white_nits, out.ctypes.data, out.size))
    return out


def colour_matrix(primaries: int) -> np.ndarray:
    """The CICP ingest's 3 x 3 matrix from `primaries` to BT.709 / sRGB primaries (ce_colour_matrix), float32."""
    out = np.empty((3, 3), np.float32)
    _host_check(lib().ce_colour_matrix(primaries, out.ctypes.data))
    return out


ICC_SUPPORTED, ICC_LUT_BASED, ICC_NOT_RGB_XYZ, ICC_MALFORMED = 0, 1, 2, 3


@dataclass(frozen=True)
class IccCurve:
    """One tone curve of a matrix/TRC profile (ce_icc_curve): type 0 `curv` (count samples; 0 the identity, 1 a gamma whose
    u8Fixed8 number is params[0]) or 1 `para` (count = the function type 0 .. 4, params = g a b c d e f as s15Fixed16)."""
    type: int
    count: int
    params: Tuple[int, ...]
    offset: int


@dataclass(frozen=True)
class IccDescription:
    """What the library's parser reads from an ICC profile (ce_icc_describe): kind 0 supported, 1 LUT-based, 2 not RGB / XYZ,
    3 malformed, with the reason; the version, the class, the nine colorant integers (rows X Y Z, columns r g b) and the
    three curves as far as parsing got."""
    kind: int
    version: int
    profile_class: int
    colorants: Tuple[int, ...]
    curves: Tuple[IccCurve, ...]
    reason: str


def icc_describe(profile: bytes) -> IccDescription:
    """ce_icc_describe: a pure host function, usable with no GPU."""
    b = bytes(profile)
    d = CeIccDescription()
    _host_check(lib().ce_icc_describe(b, len(b), C.byref(d)))
    return IccDescription(d.kind, d.version, d.profile_class, tuple(d.colorants),
                          tuple(IccCurve(c.type, c.count, tuple(c.params), c.offset) for c in d.curves), d.reason.decode(errors="replace"))


def icc_matrix(profile: bytes) -> np.ndarray:
    """The 3 x 3 float32 matrix from a matrix/TRC profile's colorants to sRGB primaries (ce_icc_build_matrix)."""
    b = bytes(profile)
    out = np.empty((3, 3), np.float32)
    if lib().ce_icc_build_matrix(b, len(b), out.ctypes.data) != CE_OK:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "ICC profile: " + (icc_describe(b).reason or "bad argument"))
    return out


def icc_tables(profile: bytes, depth: int) -> np.ndarray:
    """The three tone tables of a matrix/TRC profile at `depth` bits, [3, 2^depth] float32 (ce_icc_build_tables)."""
    b = bytes(profile)
    out = np.empty((3, 1 << depth if 0 < depth <= 16 else 1), np.float32)
    if lib().ce_icc_build_tables(b, len(b), depth, out.ctypes.data, out.size) != CE_OK:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "ICC profile: " + (icc_describe(b).reason or f"depth {depth} or the table size"))
    return out


ICC_LUT_SUPPORTED, ICC_LUT_NOT_LUT, ICC_LUT_UNSUPPORTED, ICC_LUT_MALFORMED = 0, 1, 2, 3
ICC_CLUT_TRILINEAR, ICC_CLUT_TETRAHEDRAL = 0, 1
ICC_STAGE_A, ICC_STAGE_CLUT, ICC_STAGE_M, ICC_STAGE_MATRIX, ICC_STAGE_B = 1, 2, 4, 8, 16
ICC_LUT_CURVE_IDENTITY, ICC_LUT_CURVE_SAMPLED, ICC_LUT_CURVE_POWER = 0, 1, 2


@dataclass(frozen=True)
class IccLutDescription:
    """What the library's parser reads from a LUT-based ICC profile (ce_icc_lut_describe): kind 0 supported, 1 not LUT-based,
    2 not RGB / a PCS, class or channel count not taken, 3 malformed, with the reason; the tag used, its type and the PCS as
    four-character signatures; the ICC_STAGE_* present, the grid, the CLUT's bytes per sample, the matrix's integers and the A,
    M and B curves (input and output tables for mft*: type 0 with u16, type 2 with u8 samples at `offset`)."""
    kind: int
    version: int
    profile_class: int
    pcs: bytes
    tag: bytes
    tag_type: bytes
    tag_offset: int
    tag_size: int
    stages: int
    grid: Tuple[int, ...]
    precision: int
    clut_offset: int
    matrix: Tuple[int, ...]
    a: Tuple[IccCurve, ...]
    m: Tuple[IccCurve, ...]
    b: Tuple[IccCurve, ...]
    reason: str


@dataclass(frozen=True)
class IccLutCurve:
    """A post-CLUT curve as the kernel takes it (ce_icc_lut_curve): kind 0 identity, 1 sampled (its float32 samples), 2 a power
    (the para function type and g a b c d e f as floats)."""
    kind: int
    ftype: int
    samples: Optional[np.ndarray]
    q: Tuple[float, ...]


def _sig(v: int) -> bytes:
    return int(v).to_bytes(4, "big") if v else b""


def icc_lut_describe(profile: bytes, intent: int = 0) -> IccLutDescription:
    """ce_icc_lut_describe: a pure host function, usable with no GPU."""
    b = bytes(profile)
    d = CeIccLutDescription()
    _host_check(lib().ce_icc_lut_describe(b, len(b), intent, C.byref(d)))
    curves = lambda cs: tuple(IccCurve(c.type, c.count, tuple(c.params), c.offset) for c in cs)
    return IccLutDescription(d.kind, d.version, d.profile_class, _sig(d.pcs), _sig(d.tag), _sig(d.tag_type), d.tag_offset, d.tag_size, d.stages,
                             tuple(d.grid), d.precision, d.clut_offset, tuple(d.matrix), curves(d.a), curves(d.m), curves(d.b),
                             d.reason.decode(errors="replace"))


def _icc_lut_refused(b: bytes, intent: int, what: str) -> "CodecEvalError":
    reason = icc_lut_describe(b, intent).reason if 0 <= intent <= 2 else ""
    return CodecEvalError(CE_ERR_INVALID_ARG, "ICC profile: " + (reason or what))


def icc_lut_input_tables(profile: bytes, depth: int, intent: int = 0) -> np.ndarray:
    """The three input-side tables of a LUT-based profile at `depth` bits, [3, 2^depth] float32 (ce_icc_lut_build_input_tables)."""
    b = bytes(profile)
    out = np.empty((3, 1 << depth if 0 < depth <= 16 else 1), np.float32)
    if lib().ce_icc_lut_build_input_tables(b, len(b), intent, depth, out.ctypes.data, out.size) != CE_OK:
        raise _icc_lut_refused(b, intent, f"depth {depth} or the table size")
    return out


def icc_lut_clut(profile: bytes, intent: int = 0) -> Optional[np.ndarray]:
    """The CLUT's nodes as the device holds them, [g0 * g1 * g2, 4] float32 with the fourth 0 (ce_icc_lut_build_clut); None for a
    profile without a CLUT."""
    b = bytes(profile)
    d = icc_lut_describe(b, intent)
    if d.kind != 0:
        raise _icc_lut_refused(b, intent, "bad argument")
    if not d.stages & ICC_STAGE_CLUT:
        return None
    out = np.empty((d.grid[0] * d.grid[1] * d.grid[2], 4), np.float32)
    if lib().ce_icc_lut_build_clut(b, len(b), intent, out.ctypes.data, out.size) != CE_OK:
        raise _icc_lut_refused(b, intent, "bad argument")
    return out


def icc_lut_matrix(profile: bytes, intent: int = 0) -> np.ndarray:
    """The 12 float32 numbers of the mAB matrix, 3 x 3 row-major then the offsets (ce_icc_lut_build_matrix)."""
    b = bytes(profile)
    out = np.empty(12, np.float32)
    if lib().ce_icc_lut_build_matrix(b, len(b), intent, out.ctypes.data) != CE_OK:
        raise _icc_lut_refused(b, intent, "bad argument")
    return out


def icc_lut_curves(profile: bytes, intent: int = 0) -> Tuple[IccLutCurve, ...]:
    """The six post-CLUT curves, M then B / output tables (ce_icc_lut_build_curves)."""
    b = bytes(profile)
    cs = (CeIccLutCurve * 6)()
    needed = C.c_size_t()
    rc = lib().ce_icc_lut_build_curves(b, len(b), intent, cs, None, 0, C.byref(needed))
    if rc not in (CE_OK, CE_ERR_BAD_LENGTH):
        raise _icc_lut_refused(b, intent, "bad argument")
    samples = np.empty(needed.value, np.float32)
    _host_check(lib().ce_icc_lut_build_curves(b, len(b), intent, cs, samples.ctypes.data, samples.size, C.byref(needed)))
    return tuple(IccLutCurve(c.kind, c.ftype, samples[c.first_sample:c.first_sample + c.count].copy() if c.kind == ICC_LUT_CURVE_SAMPLED else None,
                             tuple(c.q)) for c in cs)


def icc_lut_pcs_matrix() -> np.ndarray:
    """The 3 x 3 float32 matrix from PCS XYZ to linear light with sRGB primaries (ce_icc_lut_build_pcs_matrix)."""
    out = np.empty((3, 3), np.float32)
    _host_check(lib().ce_icc_lut_build_pcs_matrix(out.ctypes.data))
    return out


def srgb_encode_thresholds(depth: int) -> np.ndarray:
    """T[1 .. 2^depth - 1] of the sRGB encode of integer slots (ce_srgb_encode_thresholds), float32."""
    out = np.empty((1 << depth) - 1 if 0 < depth <= 16 else 1, np.float32)
    if lib().ce_srgb_encode_thresholds(depth, out.ctypes.data, out.size) != CE_OK:
        raise CodecEvalError(CE_ERR_INVALID_ARG, f"ce_srgb_encode_thresholds: depth 8, 10, 12 or 16, got {depth}")
    return out


@dataclass(frozen=True)
class ColourDescription:
    """How integer RGB code values are to be read (ce_colour): H.273 colour primaries (1 BT.709, 9 BT.2020, 12 Display P3)
    and transfer characteristics (13 sRGB, 8 linear, 16 PQ), bits per sample, and for PQ the luminance that becomes 1.0."""
    primaries: int = PRIMARIES_BT709
    transfer: int = TRANSFER_SRGB
    depth: int = 8
    white_nits: float = 203.0

    def with_depth(self, depth: int) -> "ColourDescription":
        return ColourDescription(self.primaries, self.transfer, depth, self.white_nits)

    @property
    def is_srgb(self) -> bool:
        return self.primaries == PRIMARIES_BT709 and self.transfer == TRANSFER_SRGB

    def _c(self) -> CeColour:
        return CeColour(self.primaries, self.transfer, self.depth, self.white_nits)


ColourDescription.SRGB = ColourDescription(PRIMARIES_BT709, TRANSFER_SRGB, 8)
ColourDescription.DISPLAY_P3 = ColourDescription(PRIMARIES_P3_D65, TRANSFER_SRGB, 8)
ColourDescription.BT2020_PQ = ColourDescription(PRIMARIES_BT2020, TRANSFER_PQ, 10, 203.0)


@dataclass(frozen=True)
class HlgDescription:
    """How BT.2100 HLG code values are to be read (ce_hlg): H.273 colour primaries (BT.2100 itself: 9), bits per sample, the
    display's nominal peak luminance L_W, the system gamma (0: BT.2100's rule from the peak) and the luminance that becomes
    1.0.  Accepted wherever a ColourDescription is; the image is scored in linear light."""
    primaries: int = PRIMARIES_BT2020
    depth: int = 10
    peak_nits: float = 1000.0
    system_gamma: float = 0.0
    white_nits: float = 203.0

    def with_depth(self, depth: int) -> "HlgDescription":
        return HlgDescription(self.primaries, depth, self.peak_nits, self.system_gamma, self.white_nits)

    @property
    def is_srgb(self) -> bool:
        return False

    def _c(self) -> CeHlg:
        return CeHlg(self.primaries, self.depth, self.peak_nits, self.system_gamma, self.white_nits)


HlgDescription.BT2100_HLG = HlgDescription()


def hlg_table(depth: int) -> np.ndarray:
    """The HLG ingest's inverse-OETF table of code value -> scene light in [0, 1] (ce_hlg_table), float32."""
    out = np.empty(1 << depth if 0 < depth <= 16 else 1, np.float32)
    _host_check(lib().ce_hlg_table(depth, out.ctypes.data, out.size))
    return out


def hlg_params(description: "HlgDescription") -> np.ndarray:
    """kR, kG, kB, gamma - 1 and A = peak_nits / white_nits of a description (ce_hlg_params), float64: exactly what the
    kernel is handed."""
    out = np.empty(5, np.float64)
    c = description._c()
    _host_check(lib().ce_hlg_params(C.byref(c), out.ctypes.data_as(_dp)))
    return out


def _three(v) -> tuple:
    """one number for all three channels, or three"""
    return tuple(float(x) for x in v) if isinstance(v, (tuple, list, np.ndarray)) else (float(v),) * 3


@dataclass(frozen=True, eq=False)
class GainMap:
    """A gain map and its metadata (ce_gainmap_image, ce_gainmap): `samples` uint8 [gh, gw] or [gh, gw, 1 or 3], at most the
    base image's size; log2 gains, the map's gamma and the two offsets as one number or three; the log2 headrooms of the
    base and the alternate rendition and the one to render for (default: the alternate's, the full HDR rendition).  With a
    single-channel map only the first of each three is read."""
    samples: np.ndarray
    gain_min: tuple = 0.0
    gain_max: tuple = 1.0
    gamma: tuple = 1.0
    base_offset: tuple = 1.0 / 64.0
    alternate_offset: tuple = 1.0 / 64.0
    base_headroom: float = 0.0
    alternate_headroom: float = 1.0
    display_headroom: Optional[float] = None

    def __post_init__(self):
        a = np.ascontiguousarray(self.samples)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise CodecEvalError(CE_ERR_INVALID_ARG, "GainMap: samples must be uint8 [gh, gw] or [gh, gw, channels]")
        object.__setattr__(self, "samples", a if a.ndim == 3 else a[..., None])
        for name in ("gain_min", "gain_max", "gamma", "base_offset", "alternate_offset"):
            object.__setattr__(self, name, _three(getattr(self, name)))
        if self.display_headroom is None:
            object.__setattr__(self, "display_headroom", self.alternate_headroom)

    @property
    def channels(self) -> int:
        return self.samples.shape[2]

    def with_samples(self, samples) -> "GainMap":
        return replace(self, samples=samples)

    def _meta(self) -> CeGainmap:
        f3 = lambda v: (C.c_float * 3)(*v)  # noqa: E731
        return CeGainmap(f3(self.gain_min), f3(self.gain_max), f3(self.gamma), f3(self.base_offset), f3(self.alternate_offset),
                         self.base_headroom, self.alternate_headroom, self.display_headroom)

    def _c(self):
        """(ce_gainmap_image, ce_gainmap); the image points into self.samples"""
        gh, gw, ch = self.samples.shape
        return CeGainmapImage(self.samples.ctypes.data, gw, gh, ch), self._meta()


def gainmap_weight(gain_map: "GainMap") -> float:
    """W of a gain map's metadata (ce_gainmap_weight): how far the rendered headroom lies between the base's and the alternate's."""
    out = C.c_double()
    m = gain_map._meta()
    _host_check(lib().ce_gainmap_weight(C.byref(m), C.byref(out)))
    return out.value


def gainmap_tables(gain_map: "GainMap", channels: Optional[int] = None) -> np.ndarray:
    """The gain-map ingest's tables of map sample -> log2 gain with W folded in (ce_gainmap_tables), float64 [channels, 256]:
    exactly what the kernel is handed."""
    channels = gain_map.channels if channels is None else channels
    out = np.empty((channels if channels in (1, 3) else 1, 256), np.float64)
    m = gain_map._meta()
    _host_check(lib().ce_gainmap_tables(C.byref(m), channels, out.ctypes.data_as(_dp), out.size))
    return out


HDR_FIDELITY_DEPTHS = (10, 12, 16)  # the PQ code grids ce_batch_hdr_fidelity scores on


def pq_code_thresholds(depth: int, white_nits: float = 203.0) -> np.ndarray:
    """The decision thresholds of PQ code values on linear light (ce_pq_code_thresholds), float32 [2^depth - 1]: entry c - 1
    is T[c] = PQ_EOTF((c - 0.5) / maxv) / white_nits, and a sample's code is numpy.searchsorted(T, x, side="right")."""
    out = np.empty((1 << depth) - 1 if 0 < depth <= 16 else 1, np.float32)
    _host_check(lib().ce_pq_code_thresholds(depth, white_nits, out.ctypes.data, out.size))
    return out


def hdr_fidelity_matrices() -> Tuple[np.ndarray, np.ndarray]:
    """HDR fidelity's two 3 x 3 matrices (ce_hdr_fidelity_matrices), float32: BT.2020 <- sRGB primaries, and BT.2100's
    LMS <- BT.2020."""
    a, b = np.empty((3, 3), np.float32), np.empty((3, 3), np.float32)
    _host_check(lib().ce_hdr_fidelity_matrices(a.ctypes.data, b.ctypes.data))
    return a, b


@dataclass(frozen=True)
class HdrFidelity:
    """PSNR in the PQ domain and BT.2124's Delta E ITP of one pair of a linear batch (ce_hdr_scores), with the three exact
    integers they are finished from: the sum of squared PQ code differences, and the sum and the maximum of the per-pixel
    Delta E in units of 2^-20."""
    pq_psnr: float
    delta_e_itp_mean: float
    delta_e_itp_max: float
    pq_sse: int
    itp_sum_q20: int
    itp_max_q20: int

    @staticmethod
    def from_c(s: CeHdrScores) -> "HdrFidelity":
        return HdrFidelity(s.pq_psnr, s.delta_e_itp_mean, s.delta_e_itp_max, int(s.pq_sse), int(s.itp_sum_q20), int(s.itp_max_q20))


def msssim_window() -> np.ndarray:
    """The 11-tap Gaussian window of SSIM / MS-SSIM (ce_msssim_window), float64: the library's literals."""
    out = np.empty(11, np.float64)
    _host_check(lib().ce_msssim_window(out.ctypes.data))
    return out


def msssim_levels(width: int, height: int, levels: int = 5) -> List[Tuple[int, int]]:
    """The (width, height) of every level of SSIM (levels = 1) or MS-SSIM (5) on a width x height image (ce_msssim_levels);
    raises for other `levels` and for an image too small."""
    n, w, h = np.zeros(1, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint32)
    _host_check(lib().ce_msssim_levels(width, height, levels, n.ctypes.data, w.ctypes.data, h.ctypes.data))
    return [(int(w[l]), int(h[l])) for l in range(int(n[0]))]


@dataclass(frozen=True)
class MsSsim:
    """SSIM and MS-SSIM of one pair on the encoded sample values (ce_msssim_scores): the means over R, G, B, the per-channel
    values, and the exact integers they are finished from - per level and channel the sums of the per-position SSIM and
    contrast-structure values in units of 2^-32 - with the positions n of every level.  ms_ssim is NaN with one level."""
    ms_ssim: float
    ssim: float
    ms_ssim_rgb: Tuple[float, float, float]
    ssim_rgb: Tuple[float, float, float]
    ssim_q: Tuple[Tuple[int, int, int], ...]
    cs_q: Tuple[Tuple[int, int, int], ...]
    n: Tuple[int, ...]
    n_levels: int

    @staticmethod
    def from_c(s: CeMsssimScores) -> "MsSsim":
        return MsSsim(s.ms_ssim, s.ssim, tuple(s.ms_ssim_rgb), tuple(s.ssim_rgb),
                      tuple(tuple(int(v) for v in s.ssim_q[l]) for l in range(5)),
                      tuple(tuple(int(v) for v in s.cs_q[l]) for l in range(5)), tuple(int(v) for v in s.n), int(s.n_levels))


CIEDE2000_Q20 = 1 << 20  # a CIEDE2000 of 1.0 in the units of q and of the thresholds (CE_CIEDE2000_Q20)
CIEDE2000_MAX_THRESHOLDS = 8  # CE_CIEDE2000_MAX_THRESHOLDS


@dataclass(frozen=True)
class Ciede2000:
    """CIEDE2000 of one pair read as sRGB (ce_ciede2000_scores): the mean and the maximum of the per-pixel Delta E 2000, the
    PSNR-like 45 - 20 log10(mean) (inf for a mean of 0), and the exact integers they are finished from - the sum and the maximum
    of the per-pixel values in units of 2^-20 over n pixels - with n_above[k], the pixels above the k-th threshold."""
    mean: float
    max: float
    ciede2000_db: float
    sum_q20: int
    max_q20: int
    n: int
    n_above: Tuple[int, ...]

    @staticmethod
    def from_c(s: CeCiede2000Scores) -> "Ciede2000":
        return Ciede2000(s.mean, s.max, s.ciede2000_db, int(s.sum_q20), int(s.max_q20), int(s.n),
                         tuple(int(s.n_above[k]) for k in range(int(s.n_thresholds))))


def _thresholds_q20(thresholds_q20) -> np.ndarray:
    """Up to 2^32 - 1 each, as the uint32 array the C calls take (more than eight are the library's to refuse)."""
    return np.ascontiguousarray(np.asarray(() if thresholds_q20 is None else thresholds_q20, np.uint64).reshape(-1).astype(np.uint32))


def ciede2000_pixels(reference, test, ref_depth: int = 8, test_depth: int = 8) -> np.ndarray:
    """The per-pixel CIEDE2000 in units of 2^-20 (ce_ciede2000_pixels), uint32 [n]: reference and test hold n * 3 integer samples
    of ref_depth / test_depth bits.  A pure host function - the kernel's pixel text compiled for the host - that needs no GPU."""
    r = np.ascontiguousarray(np.asarray(reference).astype(np.uint16).reshape(-1))
    t = np.ascontiguousarray(np.asarray(test).astype(np.uint16).reshape(-1))
    if r.size != t.size or r.size % 3:
        raise ValueError("ciede2000_pixels: both sides need the same number of RGB triples")
    out = np.empty(r.size // 3, np.uint32)
    _host_check(lib().ce_ciede2000_pixels(r.ctypes.data, ref_depth, t.ctypes.data, test_depth, out.size, out.ctypes.data))
    return out


# which of a pixel's four values a CIEDE2000 map holds (CE_CIEDE2000_MAP_*): q itself, or the magnitude of its lightness, chroma
# or hue term, all in units of 2^-20
CIEDE2000_MAP_DE, CIEDE2000_MAP_DL, CIEDE2000_MAP_DC, CIEDE2000_MAP_DH = 0, 1, 2, 3
_CIEDE2000_MAP_WHAT = {"de": CIEDE2000_MAP_DE, "dl": CIEDE2000_MAP_DL, "dc": CIEDE2000_MAP_DC, "dh": CIEDE2000_MAP_DH}


def ciede2000_pixel_terms(reference, test, ref_depth: int = 8, test_depth: int = 8) -> np.ndarray:
    """The four per-pixel values of the CIEDE2000 maps in units of 2^-20 (ce_ciede2000_pixel_terms), uint32 [n, 4]: column
    CIEDE2000_MAP_DE is ciede2000_pixels' q, columns _DL, _DC and _DH the magnitudes of the lightness, chroma and hue terms.
    A pure host function - the kernel's pixel text compiled for the host - that needs no GPU."""
    r = np.ascontiguousarray(np.asarray(reference).astype(np.uint16).reshape(-1))
    t = np.ascontiguousarray(np.asarray(test).astype(np.uint16).reshape(-1))
    if r.size != t.size or r.size % 3:
        raise ValueError("ciede2000_pixel_terms: both sides need the same number of RGB triples")
    out = np.empty((r.size // 3, 4), np.uint32)
    _host_check(lib().ce_ciede2000_pixel_terms(r.ctypes.data, ref_depth, t.ctypes.data, test_depth, out.shape[0], out.ctypes.data))
    return out


def _ciede2000_map(ctx: "Context", call, count: int, width: int, height: int, what, block: int, thresholds_q20, maps: bool):
    """The outputs of ce_batch_ciede2000_map / ce_eval_pair_ciede2000_map{,_deep} around call(what, map, map_len, thresholds, n,
    over): (uint32 [count, ceil(h / block), ceil(w / block)] or None, uint64 [count, n] or None).  what: "de", "dl", "dc", "dh"
    or a CIEDE2000_MAP_* integer, which the library checks."""
    if isinstance(what, str):
        if what not in _CIEDE2000_MAP_WHAT:
            raise CodecEvalError(CE_ERR_INVALID_ARG, 'what must be "de", "dl", "dc" or "dh"')
        what = _CIEDE2000_MAP_WHAT[what]
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    m = np.empty((max(count, 0), -(-height // block), -(-width // block)), np.uint32) if maps else None
    thr = None if thresholds_q20 is None else _thresholds_q20(thresholds_q20)
    over = None if thr is None else np.zeros((max(count, 0), thr.size), np.uint64)
    ctx._check(call(what, m.ctypes.data if maps and m.size else None, m.size if maps else 0,
                    thr.ctypes.data if thr is not None and thr.size else None, thr.size if thr is not None else 0,
                    over.ctypes.data if over is not None else None))
    return m, over


@dataclass(frozen=True)
class PlaneScores:
    """One pair of Y'CbCr images scored plane by plane (ce_plane_scores): index p = 0, 1, 2 is Y, Cb, Cr, each at its own
    resolution.  sse and n are the exact squared error and the sample count of a plane, psnr the planes' PSNR, psnr_weighted
    the 6:1:1 figure and psnr_overall the PSNR of the three planes' joint error.  ssim and ms_ssim are per plane, from the exact
    integers ssim_q[p][level] and cs_q[p][level] over n_pos[p][level] positions; n_levels[p] is how many levels plane p ran.
    What did not run is 0 (integers) or NaN (doubles)."""
    sse: Tuple[int, int, int]
    n: Tuple[int, int, int]
    psnr: Tuple[float, float, float]
    psnr_weighted: float
    psnr_overall: float
    ssim: Tuple[float, float, float]
    ms_ssim: Tuple[float, float, float]
    ssim_q: Tuple[Tuple[int, ...], ...]
    cs_q: Tuple[Tuple[int, ...], ...]
    n_pos: Tuple[Tuple[int, ...], ...]
    n_levels: Tuple[int, int, int]
    n_planes: int

    @staticmethod
    def from_c(s: CePlaneScores) -> "PlaneScores":
        grid = lambda a: tuple(tuple(int(v) for v in a[p]) for p in range(3))  # noqa: E731
        return PlaneScores(tuple(int(v) for v in s.sse), tuple(int(v) for v in s.n), tuple(s.psnr), s.psnr_weighted, s.psnr_overall,
                           tuple(s.ssim), tuple(s.ms_ssim), grid(s.ssim_q), grid(s.cs_q), grid(s.n_pos),
                           tuple(int(v) for v in s.n_levels), int(s.n_planes))


@dataclass(frozen=True)
class PlaneHvsScores:
    """PSNR-HVS and PSNR-HVS-M of one pair of Y'CbCr images plane by plane (ce_plane_hvs_scores): index p = 0, 1, 2 is Y, Cb,
    Cr.  hvs_sum[p] and hvsm_sum[p] are the exact sums of the quantised, CSF-weighted squared DCT differences without and with
    the contrast mask (hvs_q[p] and hvsm_q[p] are the same as [low 32 bits, the rest]), n_blocks[p] the plane's 8 x 8 blocks at
    the call's step, psnr_hvs and psnr_hvsm the scores.  A plane without a block has 0 and NaN."""
    hvs_q: Tuple[Tuple[int, int], ...]
    hvsm_q: Tuple[Tuple[int, int], ...]
    n_blocks: Tuple[int, int, int]
    psnr_hvs: Tuple[float, float, float]
    psnr_hvsm: Tuple[float, float, float]
    n_planes: int
    step: int

    @property
    def hvs_sum(self) -> Tuple[int, ...]:
        return tuple(q[0] + (q[1] << 32) for q in self.hvs_q)

    @property
    def hvsm_sum(self) -> Tuple[int, ...]:
        return tuple(q[0] + (q[1] << 32) for q in self.hvsm_q)

    @staticmethod
    def from_c(s: CePlaneHvsScores) -> "PlaneHvsScores":
        pairs = lambda a: tuple((int(a[p][0]), int(a[p][1])) for p in range(3))  # noqa: E731
        return PlaneHvsScores(pairs(s.hvs_q), pairs(s.hvsm_q), tuple(int(v) for v in s.n_blocks), tuple(s.psnr_hvs), tuple(s.psnr_hvsm),
                              int(s.n_planes), int(s.step))


@dataclass(frozen=True)
class PlaneVifScores:
    """Pixel-domain VIF (VIFp) of one pair of Y'CbCr images plane by plane (ce_plane_vif_scores): index p = 0, 1, 2 is Y, Cb,
    Cr.  num_q[p][s] and den_q[p][s] are the exact sums, in units of 2^-24 nat, of the information the test and the reference
    carry at scale s + 1 over n_pos[p][s] positions; vif_scale[p][s] is their ratio and vifp[p] the ratio of the sums over the
    four scales (1.0 where the denominator is 0).  ran[p] is 1 where plane p ran; a plane that did not has 0 and NaN."""
    num_q: Tuple[Tuple[int, ...], ...]
    den_q: Tuple[Tuple[int, ...], ...]
    n_pos: Tuple[Tuple[int, ...], ...]
    vif_scale: Tuple[Tuple[float, ...], ...]
    vifp: Tuple[float, float, float]
    ran: Tuple[int, int, int]
    n_planes: int

    @staticmethod
    def from_c(s: CePlaneVifScores) -> "PlaneVifScores":
        grid = lambda a, t: tuple(tuple(t(v) for v in a[p]) for p in range(3))  # noqa: E731
        return PlaneVifScores(grid(s.num_q, int), grid(s.den_q, int), grid(s.n_pos, int), grid(s.vif_scale, float), tuple(s.vifp),
                              tuple(int(v) for v in s.ran), int(s.n_planes))


@dataclass(frozen=True)
class PlaneGmsdScores:
    """GMSD of one pair of Y'CbCr images plane by plane (ce_plane_gmsd_scores): index p = 0, 1, 2 is Y, Cb, Cr.  sum_q[p] is
    the exact sum of the gradient magnitude similarities in units of 2^-32 over n_pos[p] positions, sum_q2[p] the exact sum of
    their squares as [low 64 bits, high 64 bits] (sum_q2_int[p] is the same as one integer), max_dis[p] the largest 2^32 - q;
    gmsd[p] is the deviation (dividing by N) and gmsm[p] the mean.  A plane the subsampling lacks has 0 and NaN."""
    sum_q: Tuple[int, int, int]
    sum_q2: Tuple[Tuple[int, int], ...]
    n_pos: Tuple[int, int, int]
    gmsd: Tuple[float, float, float]
    gmsm: Tuple[float, float, float]
    max_dis: Tuple[int, int, int]
    n_planes: int

    @property
    def sum_q2_int(self) -> Tuple[int, ...]:
        return tuple(q[0] + (q[1] << 64) for q in self.sum_q2)

    @staticmethod
    def from_c(s: CePlaneGmsdScores) -> "PlaneGmsdScores":
        ints = lambda a: tuple(int(v) for v in a)  # noqa: E731
        return PlaneGmsdScores(ints(s.sum_q), tuple((int(s.sum_q2[p][0]), int(s.sum_q2[p][1])) for p in range(3)), ints(s.n_pos),
                               tuple(s.gmsd), tuple(s.gmsm), ints(s.max_dis), int(s.n_planes))


def vif_window(scale: int) -> np.ndarray:
    """The Gaussian window of VIFp's scale 1 .. 4 (ce_vif_window), 17, 9, 5 or 3 float64: the library's literals."""
    out = np.empty(17, np.float64)
    _host_check(lib().ce_vif_window(scale, out.ctypes.data))
    return out[:(17, 9, 5, 3)[scale - 1]].copy()


DELTA_E_ITP_Q20 = 1 << 20  # a Delta E ITP of 1.0 in the units of the maps and thresholds (CE_DELTA_E_ITP_Q20)
DELTA_E_ITP_MAX_THRESHOLDS = 8  # CE_DELTA_E_ITP_MAX_THRESHOLDS


def _delta_e_itp_map(ctx: "Context", call, count: int, width: int, height: int, block: int, thresholds_q20, maps: bool):
    """The outputs of ce_batch_delta_e_itp_map / ce_eval_pair_delta_e_itp_map around call(map, map_len, thresholds, n, over):
    (uint32 [count, ceil(h / block), ceil(w / block)] or None, uint64 [count, n] or None)."""
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    m = np.empty((count, -(-height // block), -(-width // block)), np.uint32) if maps else None
    thr = None if thresholds_q20 is None else np.ascontiguousarray(thresholds_q20, dtype=np.uint32).reshape(-1)
    over = None if thr is None else np.zeros((count, thr.size), np.uint64)
    ctx._check(call(m.ctypes.data if maps else None, m.size if maps else 0, thr.ctypes.data if thr is not None and thr.size else None,
                    thr.size if thr is not None else 0, over.ctypes.data if over is not None else None))
    return m, over


MSSSIM_Q32 = 1 << 32  # an SSIM of 1.0 in the units of the SSIM / MS-SSIM maps and their thresholds (CE_MSSSIM_Q32)
MSSSIM_MAP_MAX_THRESHOLDS = 8  # CE_MSSSIM_MAP_MAX_THRESHOLDS
_MSSSIM_MAP_WHAT = {"ssim": 0, "cs": 1}  # CE_MSSSIM_MAP_SSIM, CE_MSSSIM_MAP_CS


def _msssim_map(ctx: "Context", call, count: int, width: int, height: int, levels: int, level: int, what: str, block: int,
                thresholds_q32, maps: bool):
    """The outputs of ce_batch_msssim_map / ce_eval_pair_msssim_map{,_deep} around call(what, map, map_len, thresholds, n, over):
    (uint32 [count, 3, ceil(vh / block), ceil(vw / block)] or None, uint64 [count, 3, n] or None), vw x vh the level's valid
    region.  What the library refuses (levels, level, the image's size) it refuses itself: the map is then empty."""
    if what not in _MSSSIM_MAP_WHAT:
        raise CodecEvalError(CE_ERR_INVALID_ARG, 'what must be "ssim" or "cs"')
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    vw = vh = 0
    if levels in (1, 5) and 0 <= level < levels and (min(width, height) >= 11 if levels == 1 else min(width, height) > 160):
        w, h = width, height
        for _ in range(level):
            w, h = (w + (w & 1)) // 2, (h + (h & 1)) // 2
        vw, vh = w - 10, h - 10
    m = np.empty((max(count, 0), 3, -(-vh // block), -(-vw // block)), np.uint32) if maps else None
    thr = None if thresholds_q32 is None else np.ascontiguousarray(thresholds_q32, dtype=np.uint32).reshape(-1)
    over = None if thr is None else np.zeros((max(count, 0), 3, thr.size), np.uint64)
    ctx._check(call(_MSSSIM_MAP_WHAT[what], m.ctypes.data if maps and m.size else None, m.size if maps else 0,
                    thr.ctypes.data if thr is not None and thr.size else None, thr.size if thr is not None else 0,
                    over.ctypes.data if over is not None else None))
    return m, over


def _cicp_fmt(a: np.ndarray) -> int:
    """The CE_PIXEL_* format of an [h, w, 3 or 4] (or flat RGB) uint8 / uint16 array."""
    alpha = a.ndim == 3 and a.shape[-1] == 4
    if a.dtype == np.uint8:
        return PIXEL_RGBA8 if alpha else PIXEL_RGB8
    if a.dtype == np.uint16:
        return PIXEL_RGBA16 if alpha else PIXEL_RGB16
    raise TypeError("CICP ingest takes uint8 or uint16 samples")


def _buf_f32(a) -> np.ndarray:
    """Borrowed view as a flat contiguous float32 array (the packed samples of a linear image)."""
    arr = np.asarray(a)
    if arr.dtype != np.float32:
        raise TypeError("linear pixel buffers must be float32")
    return np.ascontiguousarray(arr).reshape(-1)


def _buf16(a) -> np.ndarray:
    """Borrowed view as a flat contiguous u16 array (the packed samples of a deep image)."""
    arr = np.asarray(a)
    if arr.dtype != np.uint16:
        raise TypeError("deep pixel buffers must be uint16")
    return np.ascontiguousarray(arr).reshape(-1)


def scale_background(rgb8: Sequence[int], depth: int) -> Tuple[int, ...]:
    """An 8-bit background colour at `depth` bits: (v * m + 127) // 255 per sample, m = 2^depth - 1."""
    m = (1 << depth) - 1
    if any(not 0 <= int(v) <= 255 for v in rgb8) or len(rgb8) != 3:
        raise ValueError(f"a background is three 8-bit values, got {tuple(rgb8)}")
    return tuple((int(v) * m + 127) // 255 for v in rgb8)


def composite_over(rgba, background: Sequence[int], depth: int = 8) -> np.ndarray:
    """The device's alpha compositing on the host (include/ce_metrics.h: ce_batch_set_*_over), for the paths that have no
    device: straight alpha, source-over onto the opaque colour `background` (three samples of `depth` bits), on the encoded
    values, (c a + bg (m - a) + (m >> 1)) // m in exact integers.  rgba: (..., 4) uint8 (depth 8) or uint16; returns
    (..., 3) of the same type."""
    a = np.asarray(rgba)
    if a.dtype not in (np.uint8, np.uint16) or a.shape[-1] != 4:
        raise TypeError("composite_over takes (..., 4) uint8 or uint16 samples")
    if a.dtype == np.uint8 and depth != 8:
        raise ValueError("uint8 samples are depth 8")
    m = (1 << depth) - 1
    bg = np.asarray([int(v) for v in background], np.uint64)
    if bg.shape != (3,) or int(bg.max()) > m:
        raise ValueError(f"a background is three samples of at most {m}, got {tuple(background)}")
    v = np.minimum(a.astype(np.uint64), m)
    c, al = v[..., :3], v[..., 3:4]
    return ((c * al + bg * (m - al) + (m >> 1)) // m).astype(a.dtype)


def alpha_table(depth: int) -> np.ndarray:
    """The linear-light composite's coverage table of `depth` bits (ce_alpha_table): float32(k) / float32(2^depth - 1)."""
    out = np.empty(1 << depth if 0 < depth <= 16 else 1, np.float32)
    _host_check(lib().ce_alpha_table(depth, out.ctypes.data, out.size))
    return out


def _backgrounds_linear(backgrounds) -> np.ndarray:
    """[n_bg][3] linear-light background colours as the contiguous float32 array the ABI takes"""
    b = np.asarray(backgrounds, dtype=np.float32)
    if b.ndim != 2 or b.shape[1] != 3:
        raise ValueError("backgrounds are rows of three linear-light values")
    return np.ascontiguousarray(b)


def _rgba_f32(pixels) -> np.ndarray:
    a = np.asarray(pixels)
    if a.dtype != np.float32 or a.shape[-1] != 4:
        raise TypeError("PIXEL_RGBA_F32 takes (..., 4) float32 samples")
    return np.ascontiguousarray(a)


def _backgrounds(backgrounds) -> np.ndarray:
    """[n_bg][3] background samples as the contiguous u16 array the ABI takes"""
    b = np.asarray(backgrounds)
    if b.ndim != 2 or b.shape[1] != 3 or b.min(initial=0) < 0 or b.max(initial=0) > 0xffff:
        raise ValueError("backgrounds are rows of three samples")
    return np.ascontiguousarray(b, dtype=np.uint16)


def yuv_coefficients(matrix: int, range: int, depth_in: int, depth_out: int) -> Tuple[int, ...]:
    """(KY, KRV, KGU, KGV, KBU, y0, c0): the fixed-point Y'CbCr -> RGB coefficients of ce_yuv_coefficients (a pure host
    function, works without a device); raises for an unknown matrix / range or a depth outside the supported ones."""
    out = (C.c_int64 * 7)()
    rc = lib().ce_yuv_coefficients(matrix, range, depth_in, depth_out, C.byref(out))
    if rc != CE_OK:
        _raise(rc, f"yuv_coefficients: bad matrix {matrix}, range {range} or depths {depth_in} -> {depth_out}")
    return tuple(int(v) for v in out)


@dataclass
class YuvImage:
    """A decoder's Y'CbCr planes (struct ce_yuv_image).  `planes`: 2-D numpy arrays (uint8 at depth 8, uint16 above; a row
    stride beyond the row is kept as the pitch), or integer device addresses with `pitches` in bytes and
    memory=MEM_DEVICE.  PLANAR: (Y, Cb, Cr); SEMIPLANAR: (Y, interleaved CbCr); 4:0:0: (Y,)."""
    planes: Sequence
    subsampling: int = YUV_420
    layout: int = YUV_PLANAR
    matrix: int = YUV_BT601
    range: int = YUV_FULL
    upsample: int = CHROMA_TRIANGLE
    depth: int = 8
    msb_aligned: bool = False
    memory: int = MEM_HOST
    pitches: Optional[Sequence[int]] = None

    def _c(self):
        """(CeYuvImage, the arrays it borrows)"""
        c = CeYuvImage()
        keep = []
        for i, p in enumerate(list(self.planes)[:3]):
            if p is None:
                continue
            if isinstance(p, (int, np.integer)):
                c.plane[i] = int(p)
                c.pitch[i] = int(self.pitches[i]) if self.pitches is not None else 0
                continue
            a = np.asarray(p)
            if a.ndim != 2 or a.dtype not in (np.uint8, np.uint16):
                raise TypeError("a Y'CbCr plane is a 2-D uint8 or uint16 array")
            if a.shape[1] > 1 and a.strides[1] != a.itemsize:
                a = np.ascontiguousarray(a)
            keep.append(a)
            c.plane[i] = a.ctypes.data
            c.pitch[i] = int(self.pitches[i]) if self.pitches is not None else (a.strides[0] if a.shape[0] > 1 else a.shape[1] * a.itemsize)
        c.subsampling, c.layout, c.matrix, c.range = self.subsampling, self.layout, self.matrix, self.range
        c.upsample, c.depth, c.msb_aligned, c.memory = self.upsample, self.depth, int(bool(self.msb_aligned)), self.memory
        c.lut = None
        return c, keep


_TENSOR_DTYPES = {"uint8": DTYPE_U8, "uint16": DTYPE_U16, "float16": DTYPE_F16, "half": DTYPE_F16, "bfloat16": DTYPE_BF16, "float32": DTYPE_F32,
                  "float": DTYPE_F32}
_TENSOR_LAYOUTS = {"CHW": (None, 0, 1, 2), "HWC": (None, 2, 0, 1), "NCHW": (0, 1, 2, 3), "NHWC": (0, 3, 1, 2)}  # the axes of n, c, y, x


def _tensor_dtype(dtype) -> int:
    """enum ce_dtype of a numpy or a framework dtype, recognised by name ("torch.bfloat16" -> DTYPE_BF16)"""
    name = str(getattr(dtype, "name", dtype)).rsplit(".", 1)[-1]
    if name not in _TENSOR_DTYPES:
        raise TypeError(f"a tensor image is uint8, uint16, float16, bfloat16 or float32, got {dtype}")
    return _TENSOR_DTYPES[name]


class TensorImage:
    """A framework's image tensor as the library reads it (struct ce_tensor_image): the address of element (0, 0, 0, 0), the
    strides of n, c, y, x in elements, the dtype and where the memory is.  `count` images of `width` x `height`.  Built by
    from_array; it keeps the array or tensor alive, and a device tensor must stay unchanged until the batch's next launch
    has been collected."""

    def __init__(self, data: int, strides: Sequence[int], count: int, height: int, width: int, dtype: int, memory: int = MEM_HOST,
                 quantise: int = QUANT_NEAREST_EVEN, keep=None, layout: Optional[str] = None):
        self.data, self.strides = int(data), tuple(int(s) for s in strides)
        self.count, self.height, self.width = int(count), int(height), int(width)
        self.dtype, self.memory, self.quantise = int(dtype), int(memory), int(quantise)
        self.keep, self.layout = keep, layout  # the array or tensor it was built from, and the names of its axes
        if len(self.strides) != 4:
            raise ValueError("a tensor image has four strides: n, c, y, x")

    @staticmethod
    def from_array(obj, layout: str = "CHW", quantise: int = QUANT_NEAREST_EVEN, dtype: Optional[int] = None) -> "TensorImage":
        """obj: a numpy array (host memory), or any object with data_ptr(), stride(), shape, dtype and is_cuda - a torch
        tensor, on the host or the device; the package itself does not import torch.  layout names obj's axes: "CHW", "HWC",
        "NCHW" or "NHWC"; the channel axis holds 3 channels, 4 (RGBA: the fourth is never read) or 1 (gray, read as all
        three).  Views are taken as they are: a crop, a permute or an expand costs nothing.  dtype: an enum ce_dtype that
        overrides the array's own (a uint16 numpy array of bfloat16 bit patterns: DTYPE_BF16)."""
        if layout not in _TENSOR_LAYOUTS:
            raise ValueError(f"layout must be one of {tuple(_TENSOR_LAYOUTS)}, got {layout!r}")
        axes = _TENSOR_LAYOUTS[layout]
        if hasattr(obj, "data_ptr") and hasattr(obj, "stride"):
            shape, strides = tuple(int(s) for s in obj.shape), tuple(int(s) for s in obj.stride())
            address, memory = int(obj.data_ptr()), MEM_DEVICE if getattr(obj, "is_cuda", False) else MEM_HOST
            dt = _tensor_dtype(obj.dtype) if dtype is None else int(dtype)
        else:
            obj = np.asarray(obj)
            dt = _tensor_dtype(obj.dtype) if dtype is None else int(dtype)
            if any(s % obj.itemsize for s in obj.strides):
                raise ValueError("the array's strides are not whole elements")
            shape, strides = obj.shape, tuple(s // obj.itemsize for s in obj.strides)
            address, memory = obj.ctypes.data, MEM_HOST
        if len(shape) != len(layout):
            raise ValueError(f"a {layout} tensor has {len(layout)} axes, got shape {shape}")
        an, ac, ay, ax = axes
        if shape[ac] not in (1, 3, 4):
            raise ValueError(f"the channel axis holds 1, 3 or 4 channels, got {shape[ac]}")
        sn, count = (0, 1) if an is None else (strides[an] if shape[an] > 1 else 0, shape[an])
        sc = 0 if shape[ac] == 1 else strides[ac]
        # the stride of an axis of length 1 is never applied and a view may report anything for it: a contiguous one is given
        sx = strides[ax] if shape[ax] > 1 else 1
        sy = strides[ay] if shape[ay] > 1 else shape[ax] * sx
        return TensorImage(address, (sn, sc, sy, sx), count, shape[ay], shape[ax], dt, memory, quantise, keep=obj, layout=layout)

    def host_elements(self) -> np.ndarray:
        """The tensor's elements on the host as [count][height][width][3]: uint8 / uint16 as they are, float dtypes widened to
        float32, which is exact.  For the host restatements (quantise_tensor); needs the object from_array was given."""
        if self.keep is None or self.layout is None:
            raise ValueError("host_elements needs a TensorImage built by from_array")
        obj = self.keep
        if hasattr(obj, "detach"):
            obj = obj.detach().cpu()
            obj = obj.numpy() if self.dtype in (DTYPE_U8, DTYPE_U16) else obj.float().numpy()
        a = np.asarray(obj)
        if a.dtype == np.uint16 and self.dtype == DTYPE_BF16:
            a = (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
        elif a.dtype == np.uint16 and self.dtype == DTYPE_F16:
            a = a.view(np.float16)
        if a.dtype == np.float16:
            a = a.astype(np.float32)
        an, ac, ay, ax = _TENSOR_LAYOUTS[self.layout]
        if an is None:
            a, an, ac, ay, ax = a[None], 0, ac + 1, ay + 1, ax + 1
        a = np.transpose(a, (an, ay, ax, ac))
        return np.repeat(a, 3, axis=-1) if a.shape[-1] == 1 else a[..., :3]

    def _c(self) -> CeTensorImage:
        c = CeTensorImage()
        c.data = self.data
        c.stride_n, c.stride_c, c.stride_y, c.stride_x = self.strides
        c.dtype, c.memory, c.quantise = self.dtype, self.memory, self.quantise
        return c


def quantise_tensor(array, depth: int = 8, quantise: int = QUANT_NEAREST_EVEN, dtype: Optional[int] = None) -> np.ndarray:
    """The tensor ingest's rule for a float dtype into an integer slot of `depth` bits, on the host in numpy (the definition of
    include/ce_metrics.h): v = f32(x) exactly; c = v > 0 ? min(v, 1) : 0; p = c * f32(2^depth - 1), one f32 multiply; rint
    (ties to even) or floor.  uint8 at depth 8, uint16 otherwise, in array's shape.  array: float16 / float32 numpy, uint16
    bit patterns with dtype=DTYPE_BF16 or DTYPE_F16, or a framework tensor (brought to the host and widened, which is exact)."""
    if depth not in DEEP_DEPTHS:
        raise ValueError(f"depth must be one of {DEEP_DEPTHS}, got {depth}")
    if quantise not in (QUANT_NEAREST_EVEN, QUANT_TRUNCATE):
        raise ValueError(f"unknown quantise rule {quantise}")
    if hasattr(array, "data_ptr") and hasattr(array, "detach"):
        array = array.detach().cpu().float().numpy()
    a = np.asarray(array)
    if dtype == DTYPE_BF16 and a.dtype == np.uint16:
        v = (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
    elif dtype == DTYPE_F16 and a.dtype == np.uint16:
        v = a.view(np.float16).astype(np.float32)
    elif a.dtype in (np.float16, np.float32):
        v = a.astype(np.float32)
    else:
        raise TypeError(f"quantise_tensor takes float16 or float32 values, or uint16 bit patterns with dtype=, got {a.dtype}")
    with np.errstate(invalid="ignore"):
        c = np.where(v > np.float32(0), np.minimum(v, np.float32(1)), np.float32(0)).astype(np.float32)
    p = (c * np.float32((1 << depth) - 1)).astype(np.float32)
    q = np.rint(p) if quantise == QUANT_NEAREST_EVEN else np.floor(p)
    return q.astype(np.uint8 if depth == 8 else np.uint16)


def version() -> str:
    return lib().ce_version().decode()


def device_count() -> int:
    return int(lib().ce_device_count())


def _buf(a) -> np.ndarray:
    """Borrowed view as a flat contiguous u8 array (copy only if the input is not already one)."""
    arr = np.asarray(a)
    if arr.dtype != np.uint8:
        raise TypeError("pixel buffers must be uint8")
    return np.ascontiguousarray(arr).reshape(-1)


def _pinned_block(address: int, nbytes: int):
    """One ce_host_alloc block as a ctypes array (buffer protocol: numpy keeps it alive through `.base`) that frees the block
    when the last array on it is gone."""
    def _free(self):
        a, self._ce_address = getattr(self, "_ce_address", 0), 0
        if a:
            lib().ce_host_free(None, a)
    cls = type("CePinnedBlock", (C.c_ubyte * nbytes,), {"__del__": _free})
    blk = cls.from_address(address)
    blk._ce_address = address
    return blk


class PairList:
    """The ce_pair_desc array of a grid, built once: (reference, test, width, height) tuples -> descriptors that borrow the
    callers' buffers (kept alive here).  Identical reference objects share one descriptor address, which is what makes
    ce_eval_batch upload a reference once for all its distorted images."""

    def __init__(self, pairs: Sequence[tuple]):
        self.n = len(pairs)
        self.descs = (CePairDesc * self.n)()
        keep = {}  # id(buffer) -> (flat view, address, length, the object): a reference shared by many pairs is looked at once

        def addr(a):
            e = keep.get(id(a))
            if e is None:
                v = _buf(a)
                e = keep[id(a)] = (v, v.__array_interface__["data"][0], v.size, a)
            return e
        for i, (ref, test, w, h) in enumerate(pairs):
            r, t, d = addr(ref), addr(test), self.descs[i]
            d.reference, d.reference_len, d.test, d.test_len, d.width, d.height = r[1], r[2], t[1], t[2], w, h
        self._keep = keep

    def __len__(self):
        return self.n


# ---- MetricConfig / MetricResult mirrors (src/metrics/mod.rs:46-149) -----------------------
@dataclass
class MetricConfig:
    dssim: bool = False
    ssimulacra2: bool = False
    butteraugli: bool = False
    psnr: bool = False
    xyb_roundtrip: bool = False

    @staticmethod
    def all() -> "MetricConfig":
        return MetricConfig(True, True, True, True, False)

    @staticmethod
    def fast() -> "MetricConfig":
        return MetricConfig(psnr=True)

    @staticmethod
    def perceptual() -> "MetricConfig":
        return MetricConfig(True, True, True, False, False)

    @staticmethod
    def perceptual_xyb() -> "MetricConfig":
        return MetricConfig(True, True, True, False, True)

    @staticmethod
    def ssimulacra2_only() -> "MetricConfig":
        return MetricConfig(ssimulacra2=True)

    def with_xyb_roundtrip(self) -> "MetricConfig":
        return MetricConfig(self.dssim, self.ssimulacra2, self.butteraugli, self.psnr, True)

    @property
    def mask(self) -> int:
        return (
            (METRIC_DSSIM if self.dssim else 0)
            | (METRIC_SSIMULACRA2 if self.ssimulacra2 else 0)
            | (METRIC_BUTTERAUGLI if self.butteraugli else 0)
            | (METRIC_PSNR if self.psnr else 0)
        )

    @property
    def flags(self) -> int:
        return FLAG_XYB_ROUNDTRIP if self.xyb_roundtrip else 0


PERCEPTION_LEVELS = ("Imperceptible", "Marginal", "Subtle", "Noticeable", "Degraded")


def perception_from_dssim(d: float) -> str:  # src/metrics/mod.rs:189-201
    for level, t in zip(PERCEPTION_LEVELS, (0.0003, 0.0007, 0.0015, 0.003)):
        if d < t:
            return level
    return "Degraded"


def perception_from_ssimulacra2(s: float) -> str:  # mod.rs:206-218
    for level, t in zip(PERCEPTION_LEVELS, (90.0, 80.0, 70.0, 50.0)):
        if s > t:
            return level
    return "Degraded"


def perception_from_butteraugli(b: float) -> str:  # mod.rs:223-235
    for level, t in zip(PERCEPTION_LEVELS, (1.0, 2.0, 3.0, 5.0)):
        if b < t:
            return level
    return "Degraded"


@dataclass
class ButteraugliResult:
    """ButteraugliResult (src/metrics/prelude.rs:64-65): the score and the per-pixel diffmap, an [h, w] float32 array."""
    score: float
    diffmap: np.ndarray


def _read_diffmaps(ctx: "Context", fn, handle, width: int, height: int, first: int, count: int, block: int) -> np.ndarray:
    """[count, ceil(h / block), ceil(w / block)] float32 through ce_batch_butteraugli_diffmap / ce_ref_butteraugli_diffmap."""
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    out = np.empty((count, -(-height // block), -(-width // block)), np.float32)
    ctx._check(fn(handle, first, count, block, out.ctypes.data, out.size))
    return out


@dataclass
class SsimMap:
    """dssim-core's SsimMap (re-exported at src/metrics/prelude.rs:45): one scale's per-pixel SSIM image, an [h_l, w_l]
    float32 array, and that scale's pooled score."""
    map: np.ndarray
    ssim: float


def dssim_levels(width: int, height: int) -> List[Tuple[int, int]]:
    """(w_l, h_l) of DSSIM's scales (Dssim::create_image): halved (floor) while at least 8 x 8, at most DSSIM_MAX_LEVELS."""
    n, lw, lh = _u32(), (_u32 * DSSIM_MAX_LEVELS)(), (_u32 * DSSIM_MAX_LEVELS)()
    L = lib()
    rc = L.ce_dssim_levels(width, height, C.byref(n), lw, lh)
    if rc != CE_OK:
        _raise(rc, (L.ce_last_error(None) or b"").decode())
    return [(int(lw[l]), int(lh[l])) for l in range(n.value)]


def _read_ssim_maps(ctx: "Context", fn, handle, width: int, height: int, level: int, first: int, count: int, block: int):
    """(maps float32 [count, ceil(h_l / block), ceil(w_l / block)], ssim float64 [count]) through ce_batch_dssim_ssim_maps /
    ce_ref_dssim_ssim_maps."""
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    levels = dssim_levels(width, height)
    if not 0 <= level < len(levels):
        raise CodecEvalError(CE_ERR_INVALID_ARG, f"DSSIM level {level} of {len(levels)}")
    w, h = levels[level]
    maps = np.empty((count, -(-h // block), -(-w // block)), np.float32)
    ssim = np.empty(count, np.float64)
    ctx._check(fn(handle, level, first, count, block, maps.ctypes.data, maps.size, ssim.ctypes.data))
    return maps, ssim


def ssimulacra2_scales(width: int, height: int) -> List[Tuple[int, int]]:
    """(w_s, h_s) of SSIMULACRA2's scales: a scale exists while its parent is at least 8 x 8 and is the parent halved with
    ceiling, at most SSIM2_MAX_SCALES (none below 8 x 8)."""
    n, sw, sh = _u32(), (_u32 * SSIM2_MAX_SCALES)(), (_u32 * SSIM2_MAX_SCALES)()
    L = lib()
    rc = L.ce_ssimulacra2_scales(width, height, C.byref(n), sw, sh)
    if rc != CE_OK:
        _raise(rc, (L.ce_last_error(None) or b"").decode())
    return [(int(sw[s]), int(sh[s])) for s in range(n.value)]


def _read_ssim2_maps(ctx: "Context", fn, handle, width: int, height: int, scale: int, channel: int, kind: int, first: int,
                     count: int, block: int, maps: bool = True):
    """(maps float32 [count, ceil(h_s / block), ceil(w_s / block)] or None, norms float64 [count, 2]) through
    ce_batch_ssimulacra2_maps / ce_ref_ssimulacra2_maps."""
    if block < 1:
        raise CodecEvalError(CE_ERR_INVALID_ARG, "block must be 1 or a power of two up to 64")
    scales = ssimulacra2_scales(width, height) if width and height else []
    if not 0 <= scale < len(scales):
        raise CodecEvalError(CE_ERR_INVALID_ARG, f"SSIMULACRA2 scale {scale} of {len(scales)}")
    w, h = scales[scale]
    m = np.empty((count, -(-h // block), -(-w // block)), np.float32) if maps else None
    norms = np.empty((count, 2), np.float64)
    ctx._check(fn(handle, scale, channel, kind, first, count, block, m.ctypes.data if maps else None, m.size if maps else 0,
                  norms.ctypes.data))
    return m, norms


@dataclass
class ImageHeuristics:
    """ImageHeuristics (crates/codec-compare/src/image_heuristics.rs:22-63) of one image, computed on the device: the
    reference's fields and order, image name included (empty unless the caller sets it), plus analyze-image's
    detail_block_pct (blocks with variance > 1000, analyze_image.rs:94-96).  The f32 fields are Python floats holding the
    exact f32 values."""
    image: str
    width: int
    height: int
    pixels: int
    mean_luminance: float
    luminance_variance: float
    luminance_std: float
    edge_strength_mean: float
    edge_strength_max: float
    edge_density: float
    flat_block_pct: float
    low_var_block_pct: float
    mid_var_block_pct: float
    high_var_block_pct: float
    detail_block_pct: float
    block_variance_mean: float
    block_variance_std: float
    color_variance: float
    saturation_mean: float
    saturation_std: float
    high_freq_energy: float
    low_freq_energy: float
    freq_ratio: float
    local_contrast_mean: float
    local_contrast_std: float
    horizontal_complexity: float
    vertical_complexity: float
    diagonal_complexity: float
    analyze_detail_block_pct: float

    @staticmethod
    def from_c(h: CeImageHeuristics, image: str = "") -> "ImageHeuristics":
        return ImageHeuristics(image, *[getattr(h, f) for f in HEURISTICS_FIELDS])


@dataclass
class MetricResult:
    dssim: Optional[float] = None
    ssimulacra2: Optional[float] = None
    butteraugli: Optional[float] = None
    psnr: Optional[float] = None

    def perception_level(self) -> Optional[str]:  # mod.rs:154-156 (DSSIM only)
        return None if self.dssim is None else perception_from_dssim(self.dssim)

    @staticmethod
    def from_c(s: CeScores) -> "MetricResult":
        return MetricResult(
            s.dssim if s.valid & METRIC_DSSIM else None,
            s.ssimulacra2 if s.valid & METRIC_SSIMULACRA2 else None,
            s.butteraugli if s.valid & METRIC_BUTTERAUGLI else None,
            s.psnr if s.valid & METRIC_PSNR else None,
        )


class Context:
    """One device + one stream (GpuSsim2::new, crates/codec-iter/src/gpu.rs:40)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        L = lib()
        rc = L.ce_ctx_create_on_stream(device, stream, C.byref(self._h)) if stream else L.ce_ctx_create(device, C.byref(self._h))
        if rc != CE_OK:
            msg = (L.ce_last_error(None) or b"").decode()
            self._h = C.c_void_p()
            _raise(rc, msg)
        self.device = device

    # -- lifetime
    def close(self):
        if self._h:
            lib().ce_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _err(self) -> str:
        return (lib().ce_last_error(self._h) or b"").decode()

    def _check(self, rc: int):
        if rc != CE_OK:
            _raise(rc, self._err())

    @property
    def stream(self) -> int:
        return int(lib().ce_ctx_stream(self._h) or 0)

    def synchronize(self):
        self._check(lib().ce_ctx_synchronize(self._h))

    def memory_info(self):
        """(free, total) device bytes."""
        free, total = C.c_size_t(), C.c_size_t()
        self._check(lib().ce_ctx_memory_info(self._h, C.byref(free), C.byref(total)))
        return free.value, total.value

    def debug_div_sweep(self, seed: int, count: int) -> int:
        """Mismatches between the shared-reciprocal division of the Malta pre-scaling and operator/ (must be 0)."""
        bad = C.c_uint64()
        self._check(lib().ce_debug_div_sweep(self._h, seed, count, C.byref(bad)))
        return bad.value

    def debug_calibrate_traffic(self, nbytes: int):
        """Run the known-byte-count calibration streams (profiles/make_traffic.py reads them from a PMC pass)."""
        self._check(lib().ce_debug_calibrate_traffic(self._h, nbytes))

    def debug_cbrt_sweep(self, first_bits: int, count: int):
        """(mismatches, fallbacks) of the fast vs reference cube root over f32 bit patterns."""
        mism, slow = C.c_uint64(), C.c_uint64()
        self._check(lib().ce_debug_cbrt_sweep(self._h, first_bits, count, C.byref(mism), C.byref(slow)))
        return mism.value, slow.value

    # -- leaf calls, same names / argument order as the reference
    def _leaf(self, fn, reference, test, width, height, *extra) -> float:
        r, t = _buf(reference), _buf(test)
        out = C.c_double()
        self._check(fn(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height, *extra, C.byref(out)))
        return out.value

    def calculate_psnr(self, reference, test, width: int, height: int) -> float:
        """calculate_psnr, src/metrics/mod.rs:312 (the reference panics on bad lengths; this raises)."""
        return self._leaf(lib().ce_calculate_psnr, reference, test, width, height)

    def calculate_ssimulacra2(self, reference, test, width: int, height: int) -> float:
        """calculate_ssimulacra2, src/metrics/ssimulacra2.rs:59."""
        return self._leaf(lib().ce_calculate_ssimulacra2, reference, test, width, height)

    def calculate_dssim(self, reference, test, width: int, height: int) -> float:
        """rgb8_to_dssim_image x2 + calculate_dssim, src/metrics/dssim.rs:102,40."""
        return self._leaf(lib().ce_calculate_dssim, reference, test, width, height)

    def calculate_butteraugli(self, reference, test, width: int, height: int) -> float:
        """calculate_butteraugli, src/metrics/butteraugli.rs:45."""
        return self._leaf(lib().ce_calculate_butteraugli, reference, test, width, height, DEFAULT_INTENSITY_TARGET)

    def calculate_butteraugli_with_intensity(self, reference, test, width: int, height: int, intensity_target: float) -> float:
        """calculate_butteraugli_with_intensity, src/metrics/butteraugli.rs:99."""
        return self._leaf(lib().ce_calculate_butteraugli, reference, test, width, height, float(intensity_target))

    def calculate_butteraugli_diffmap(self, reference, test, width: int, height: int,
                                      intensity_target: float = DEFAULT_INTENSITY_TARGET) -> ButteraugliResult:
        """calculate_butteraugli / _with_intensity returning ButteraugliResult{score, diffmap}, src/metrics/butteraugli.rs:45,99
        and src/metrics/prelude.rs:64-65: diffmap is the [h, w] float32 map whose maximum is the score."""
        r, t = _buf(reference), _buf(test)
        score = C.c_double()
        dm = np.empty((height, width), np.float32)
        self._check(lib().ce_calculate_butteraugli_diffmap(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height,
                                                           float(intensity_target), C.byref(score), dm.ctypes.data))
        return ButteraugliResult(score.value, dm)

    def calculate_dssim_with_ssim_maps(self, reference, test, width: int, height: int) -> Tuple[float, List[SsimMap]]:
        """Dssim::compare with the maps kept (Dssim::set_save_ssim_maps): (the score of calculate_dssim, one SsimMap per
        scale, level 0 = full resolution)."""
        r, t = _buf(reference), _buf(test)
        levels = dssim_levels(width, height) if width and height else []
        maps = np.empty(sum(w * h for w, h in levels), np.float32)
        ssim = np.empty(DSSIM_MAX_LEVELS, np.float64)
        score = C.c_double()
        self._check(lib().ce_calculate_dssim_ssim_maps(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height,
                                                       C.byref(score), ssim.ctypes.data, maps.ctypes.data, maps.size))
        out, off = [], 0
        for l, (w, h) in enumerate(levels):
            out.append(SsimMap(maps[off:off + w * h].reshape(h, w), float(ssim[l])))
            off += w * h
        return score.value, out

    def calculate_ssimulacra2_with_maps(self, reference, test, width: int, height: int):
        """calculate_ssimulacra2 with everything the score pools kept: (the score, features float64 [6, 3, 6] - per scale
        and XYB channel the means and 4-norms of the SSIM, artifact and detail-lost maps, NaN past the image's scales -,
        one float32 [3 channels, 3 kinds, h_s, w_s] array per scale, kinds in SSIM2_MAP_* order)."""
        r, t = _buf(reference), _buf(test)
        scales = ssimulacra2_scales(width, height) if width and height else []
        maps = np.empty(9 * sum(w * h for w, h in scales), np.float32)
        features = np.empty((SSIM2_MAX_SCALES, 3, 6), np.float64)
        score = C.c_double()
        self._check(lib().ce_calculate_ssimulacra2_maps(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height,
                                                        C.byref(score), features.ctypes.data, maps.ctypes.data, maps.size))
        out, off = [], 0
        for w, h in scales:
            out.append(maps[off:off + 9 * w * h].reshape(3, 3, h, w))
            off += 9 * w * h
        return score.value, features, out

    def xyb_roundtrip(self, rgb, width: int, height: int) -> np.ndarray:
        """xyb_roundtrip, src/metrics/xyb.rs:225."""
        r = _buf(rgb)
        out = np.empty(r.size, np.uint8)
        self._check(lib().ce_xyb_roundtrip(self._h, r.ctypes.data, r.size, width, height, out.ctypes.data))
        return out

    def rgb8_to_dssim_image(self, rgb, width: int, height: int) -> np.ndarray:
        """rgb8_to_dssim_image, src/metrics/dssim.rs:102 -> (h, w, 4) float32, a = 1.0."""
        r = _buf(rgb)
        out = np.empty((height, width, 4), np.float32)
        self._check(lib().ce_rgb8_to_dssim_image(self._h, r.ctypes.data, r.size, width, height, out.ctypes.data))
        return out

    def image_heuristics(self, rgb, width: int, height: int, image: str = "") -> ImageHeuristics:
        """compute_heuristics, crates/codec-compare/src/image_heuristics.rs:76 (images under 3 x 3 raise)."""
        r = _buf(rgb)
        out = CeImageHeuristics()
        self._check(lib().ce_image_heuristics_rgb8(self._h, r.ctypes.data, r.size, width, height, C.byref(out)))
        return ImageHeuristics.from_c(out, image)

    def resample_rgb8(self, rgb, width: int, height: int, out_width: int, out_height: int,
                      filter: int = RESAMPLE_LANCZOS3) -> np.ndarray:
        """One packed RGB8 image at another size (ce_resample_rgb8): the image SimulationParams (src/viewing.rs:308-331)
        describes, by the fixed-point separable convolution of Pillow's Image.resize, bit for bit -> (out_height,
        out_width, 3) uint8."""
        r = _buf(rgb)
        out = np.empty((max(out_height, 0), max(out_width, 0), 3), np.uint8)
        self._check(lib().ce_resample_rgb8(self._h, r.ctypes.data, r.size, width, height, out_width, out_height, filter,
                                           out.ctypes.data, out.size))
        return out

    def resample_linear(self, rgb, width: int, height: int, out_width: int, out_height: int,
                        filter: int = RESAMPLE_LANCZOS3) -> np.ndarray:
        """One packed float32 RGB image in linear light at another size (ce_resample_linear): the convolution of Pillow's
        Image.resize on mode "F" images - f64 weights and accumulator, one rounding to f32 per pass - bit for bit, clamped
        to +-LINEAR_MAX -> (out_height, out_width, 3) float32."""
        r = _buf_f32(rgb)
        out = np.empty((max(out_height, 0), max(out_width, 0), 3), np.float32)
        self._check(lib().ce_resample_linear(self._h, r.ctypes.data, r.nbytes, width, height, out_width, out_height, filter,
                                             out.ctypes.data, out.nbytes))
        return out

    def yuv_to_rgb8(self, image: "YuvImage", width: int, height: int) -> np.ndarray:
        """A decoder's Y'CbCr planes -> (height, width, 3) uint8 by the device's chroma upsampling and colour matrix
        (ce_yuv_to_rgb8; the definition is in include/ce_metrics.h)."""
        c, _keep = image._c()
        out = np.empty((height, width, 3), np.uint8)
        self._check(lib().ce_yuv_to_rgb8(self._h, C.byref(c), width, height, out.ctypes.data, out.size))
        return out

    def yuv_to_rgb16(self, image: "YuvImage", width: int, height: int, depth_out: int) -> np.ndarray:
        """The same to (height, width, 3) uint16 samples of `depth_out` bits (8, 10, 12 or 16)."""
        c, _keep = image._c()
        out = np.empty((height, width, 3), np.uint16)
        self._check(lib().ce_yuv_to_rgb16(self._h, C.byref(c), width, height, depth_out, out.ctypes.data, out.size))
        return out

    def tensor_to_rgb8(self, image: "TensorImage") -> np.ndarray:
        """Image 0 of a tensor as an RGB8 slot would hold it: (height, width, 3) uint8 (ce_tensor_to_rgb8; the definition is
        in include/ce_metrics.h)."""
        c = image._c()
        out = np.empty((image.height, image.width, 3), np.uint8)
        self._check(lib().ce_tensor_to_rgb8(self._h, C.byref(c), image.width, image.height, out.ctypes.data, out.size))
        return out

    def tensor_to_rgb16(self, image: "TensorImage", depth_out: int) -> np.ndarray:
        """The same as a deep side of depth_out bits (8, 10, 12 or 16) would: (height, width, 3) uint16 (ce_tensor_to_rgb16)."""
        c = image._c()
        out = np.empty((image.height, image.width, 3), np.uint16)
        self._check(lib().ce_tensor_to_rgb16(self._h, C.byref(c), image.width, image.height, depth_out, out.ctypes.data, out.size))
        return out

    def tensor_to_linear(self, image: "TensorImage") -> np.ndarray:
        """A float tensor as a slot of a linear batch would hold it: (height, width, 3) float32 (ce_tensor_to_linear)."""
        c = image._c()
        out = np.empty((image.height, image.width, 3), np.float32)
        self._check(lib().ce_tensor_to_linear(self._h, C.byref(c), image.width, image.height, out.ctypes.data, out.size))
        return out

    def yuv_to_linear(self, image: "YuvImage", width: int, height: int, colour: "ColourDescription") -> np.ndarray:
        """A decoder's Y'CbCr planes read by `colour` -> (height, width, 3) float32 linear light with sRGB primaries, in one
        kernel (ce_yuv_to_linear): yuv_to_rgb16 at depth_out = colour.depth followed by cicp_to_linear, bit for bit."""
        c, _keep = image._c()
        col = colour._c()
        out = np.empty((height, width, 3), np.float32)
        self._check(lib().ce_yuv_to_linear(self._h, C.byref(c), C.byref(col), width, height, out.ctypes.data, out.size))
        return out

    def yuv_icc_to_linear(self, image: "YuvImage", width: int, height: int, rgb_depth: int, profile: "IccProfile") -> np.ndarray:
        """A decoder's Y'CbCr planes read through an ICC profile of either flavour -> (height, width, 3) float32 linear light
        with sRGB primaries, in one kernel (ce_yuv_icc_to_linear): yuv_to_rgb16 at depth_out = rgb_depth followed by
        icc_to_linear at depth = rgb_depth, bit for bit.  rgb_depth: 8, 10, 12 or 16, not under the planes' depth."""
        c, _keep = image._c()
        out = np.empty((height, width, 3), np.float32)
        self._check(lib().ce_yuv_icc_to_linear(self._h, C.byref(c), rgb_depth, profile._h if profile is not None else None, width, height,
                                               out.ctypes.data, out.size))
        return out

    def yuv_icc_to_srgb(self, image: "YuvImage", width: int, height: int, rgb_depth: int, profile: "IccProfile", depth_out: int = 8) -> np.ndarray:
        """The same planes as sRGB code values: (height, width, 3) uint8 (depth_out = 8, ce_yuv_icc_to_srgb8) or uint16 of
        depth_out bits (10, 12 or 16, ce_yuv_icc_to_srgb16): yuv_to_rgb16 followed by icc_to_srgb, bit for bit."""
        c, _keep = image._c()
        h = profile._h if profile is not None else None
        if depth_out == 8:
            out = np.empty((height, width, 3), np.uint8)
            self._check(lib().ce_yuv_icc_to_srgb8(self._h, C.byref(c), rgb_depth, h, width, height, out.ctypes.data, out.size))
        else:
            out = np.empty((height, width, 3), np.uint16)
            self._check(lib().ce_yuv_icc_to_srgb16(self._h, C.byref(c), rgb_depth, h, width, height, depth_out, out.ctypes.data, out.size))
        return out

    def composite_rgba8(self, rgba, width: int, height: int, background: Sequence[int]) -> np.ndarray:
        """Straight-alpha RGBA8 source-over onto the opaque 8-bit colour `background` -> (height, width, 3) uint8, on the
        device (ce_composite_rgba8; the definition is in include/ce_metrics.h)."""
        a = _buf(rgba)
        bg = _backgrounds([background])
        if int(bg.max()) > 255:
            raise ValueError("an 8-bit background sample is at most 255")
        bg8 = bg.astype(np.uint8)
        out = np.empty((height, width, 3), np.uint8)
        self._check(lib().ce_composite_rgba8(self._h, a.ctypes.data, a.size, width, height, bg8.ctypes.data, out.ctypes.data, out.size))
        return out

    def composite_rgba16(self, rgba, width: int, height: int, depth: int, background: Sequence[int]) -> np.ndarray:
        """The same for u16 RGBA samples of `depth` bits (8, 10, 12 or 16) and a background at that depth."""
        a = _buf16(rgba)
        bg = _backgrounds([background])
        out = np.empty((height, width, 3), np.uint16)
        self._check(lib().ce_composite_rgba16(self._h, a.ctypes.data, a.size, width, height, depth, bg.ctypes.data, out.ctypes.data, out.size))
        return out

    # -- dispatcher
    def calculate_metrics(self, reference, test, width: int, height: int, config: MetricConfig,
                          intensity_target: float = DEFAULT_INTENSITY_TARGET) -> MetricResult:
        """EvalSession::calculate_metrics, src/eval/session.rs:437-497."""
        r, t = _buf(reference), _buf(test)
        s = CeScores()
        self._check(lib().ce_eval_pair(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height,
                                       config.mask, config.flags, intensity_target, C.byref(s)))
        return MetricResult.from_c(s)

    def eval_pair_deep(self, reference, ref_depth: int, test, test_depth: int, width: int, height: int, config: MetricConfig,
                       intensity_target: float = DEFAULT_INTENSITY_TARGET) -> MetricResult:
        """calculate_metrics over packed uint16 RGB at its own precision (ce_eval_pair_deep): sample v of a side of depth d
        means the sRGB value v / (2^d - 1).  PSNR is reported only for equal depths."""
        r, t = _buf16(reference), _buf16(test)
        s = CeScores()
        self._check(lib().ce_eval_pair_deep(self._h, r.ctypes.data, r.nbytes, ref_depth, t.ctypes.data, t.nbytes, test_depth, width,
                                            height, config.mask, config.flags, intensity_target, C.byref(s)))
        return MetricResult.from_c(s)

    def eval_pair_linear(self, reference, test, width: int, height: int, config: MetricConfig,
                         intensity_target: float = DEFAULT_INTENSITY_TARGET) -> MetricResult:
        """calculate_metrics over packed float32 RGB, linear light with sRGB primaries, 1.0 = the white of an 8-bit 255
        (ce_eval_pair_linear).  PSNR is not reported."""
        r, t = _buf_f32(reference), _buf_f32(test)
        s = CeScores()
        self._check(lib().ce_eval_pair_linear(self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, width, height, config.mask,
                                              config.flags, intensity_target, C.byref(s)))
        return MetricResult.from_c(s)

    def hdr_fidelity(self, reference, test, width: int, height: int, depth: int = 10, white_nits: float = 203.0) -> HdrFidelity:
        """PQ-PSNR and BT.2124 Delta E ITP of one pair of packed float32 RGB, linear light with sRGB primaries
        (ce_eval_pair_hdr_fidelity): `depth` (10, 12 or 16) is the PQ code grid, `white_nits` the luminance of 1.0."""
        r, t = _buf_f32(reference), _buf_f32(test)
        s = CeHdrScores()
        self._check(lib().ce_eval_pair_hdr_fidelity(self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, width, height, depth,
                                                    white_nits, C.byref(s)))
        return HdrFidelity.from_c(s)

    def ms_ssim(self, reference, test, width: int, height: int, levels: int = 5, depth: int = 0) -> MsSsim:
        """SSIM (levels = 1) and MS-SSIM (5) of one pair on the encoded sample values: packed uint8 RGB (depth 0;
        ce_eval_pair_msssim) or packed uint16 RGB of `depth` bits on both sides (ce_eval_pair_msssim_deep)."""
        s = CeMsssimScores()
        if depth == 0:
            r, t = _buf(reference), _buf(test)
            self._check(lib().ce_eval_pair_msssim(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height, levels, C.byref(s)))
        else:
            r, t = _buf16(reference), _buf16(test)
            self._check(lib().ce_eval_pair_msssim_deep(self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, depth, width, height,
                                                       levels, C.byref(s)))
        return MsSsim.from_c(s)

    def ciede2000(self, reference, test, width: int, height: int, thresholds_q20=None, depth: int = 0, test_depth: Optional[int] = None) -> Ciede2000:
        """CIEDE2000 of one pair read as sRGB: packed uint8 RGB (`depth` 0, ce_eval_pair_ciede2000) or packed uint16 RGB with the
        reference at `depth` and the test at `test_depth` bits (`depth` again when None; ce_eval_pair_ciede2000_deep).
        thresholds_q20: up to eight values in units of 2^-20 whose exceedance counts come back in n_above."""
        s = CeCiede2000Scores()
        thr = _thresholds_q20(thresholds_q20)
        if depth == 0:
            r, t = _buf(reference), _buf(test)
            self._check(lib().ce_eval_pair_ciede2000(self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height,
                                                     thr.ctypes.data if thr.size else None, thr.size, C.byref(s)))
        else:
            r, t = _buf16(reference), _buf16(test)
            self._check(lib().ce_eval_pair_ciede2000_deep(self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, depth,
                                                          depth if test_depth is None else test_depth, width, height,
                                                          thr.ctypes.data if thr.size else None, thr.size, C.byref(s)))
        return Ciede2000.from_c(s)

    def ciede2000_map(self, reference, test, width: int, height: int, what="de", block: int = 1, thresholds_q20=None, maps: bool = True,
                      depth: int = 0, test_depth: Optional[int] = None):
        """Batch.ciede2000_maps for one pair of packed uint8 RGB (`depth` 0; ce_eval_pair_ciede2000_map) or packed uint16 RGB with
        the reference at `depth` and the test at `test_depth` bits (`depth` again when None; ce_eval_pair_ciede2000_map_deep):
        (uint32 [1, ceil(h / block), ceil(w / block)] or None, uint64 [1, n] or None)."""
        if depth == 0:
            r, t = _buf(reference), _buf(test)
            call = lambda wh, m, n, thr, k, over: lib().ce_eval_pair_ciede2000_map(  # noqa: E731
                self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height, wh, block, m, n, thr, k, over)
        else:
            r, t = _buf16(reference), _buf16(test)
            call = lambda wh, m, n, thr, k, over: lib().ce_eval_pair_ciede2000_map_deep(  # noqa: E731
                self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, depth, depth if test_depth is None else test_depth, width, height,
                wh, block, m, n, thr, k, over)
        return _ciede2000_map(self, call, 1, width, height, what, block, thresholds_q20, maps)

    def ms_ssim_map(self, reference, test, width: int, height: int, levels: int = 5, level: int = 0, what: str = "ssim", block: int = 1,
                    thresholds_q32=None, maps: bool = True, depth: int = 0):
        """Batch.ms_ssim_maps for one pair of packed uint8 RGB (depth 0; ce_eval_pair_msssim_map) or packed uint16 RGB of `depth`
        bits on both sides (ce_eval_pair_msssim_map_deep): (uint32 [1, 3, ch, cw] or None, uint64 [1, 3, n] or None)."""
        if depth == 0:
            r, t = _buf(reference), _buf(test)
            call = lambda wh, m, n, thr, k, over: lib().ce_eval_pair_msssim_map(  # noqa: E731
                self._h, r.ctypes.data, r.size, t.ctypes.data, t.size, width, height, levels, level, wh, block, m, n, thr, k, over)
        else:
            r, t = _buf16(reference), _buf16(test)
            call = lambda wh, m, n, thr, k, over: lib().ce_eval_pair_msssim_map_deep(  # noqa: E731
                self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, depth, width, height, levels, level, wh, block, m, n, thr, k, over)
        return _msssim_map(self, call, 1, width, height, levels, level, what, block, thresholds_q32, maps)

    def plane_fidelity(self, refs: Sequence["YuvImage"], tests: Sequence["YuvImage"], width: int, height: int,
                       pair_ref: Optional[Sequence[int]] = None, levels: int = 5) -> List[PlaneScores]:
        """PSNR (levels = 0), + SSIM (1), + MS-SSIM (5) of Y'CbCr images plane by plane, on the planes as a decoder wrote
        them (ce_yuv_plane_fidelity): tests[i] against refs[pair_ref[i]], or against refs[i] without a pair table.  Every
        image is width x height with one subsampling and one depth; layout, pitch, alignment and memory are each image's
        own.  Returns once the scores are on the host; no batch is touched and device planes are only read."""
        cr, ct = (CeYuvImage * max(len(refs), 1))(), (CeYuvImage * max(len(tests), 1))()
        keep = []
        for arr, imgs in ((cr, refs), (ct, tests)):
            for i, img in enumerate(imgs):
                arr[i], k = img._c()
                keep.append(k)
        table = None if pair_ref is None else np.ascontiguousarray(pair_ref, dtype=np.uint32).reshape(-1)
        if table is not None and table.size != len(tests):
            raise CodecEvalError(CE_ERR_INVALID_ARG, f"pair_ref names {table.size} pairs for {len(tests)} tests")
        out = (CePlaneScores * max(len(tests), 1))()
        self._check(lib().ce_yuv_plane_fidelity(self._h, width, height, cr, len(refs), ct, len(tests),
                                                table.ctypes.data if table is not None else None, levels, out))
        return [PlaneScores.from_c(out[i]) for i in range(len(tests))]

    def plane_hvs(self, refs: Sequence["YuvImage"], tests: Sequence["YuvImage"], width: int, height: int,
                  pair_ref: Optional[Sequence[int]] = None, step: int = 8) -> List[PlaneHvsScores]:
        """PSNR-HVS and PSNR-HVS-M of Y'CbCr images plane by plane (ce_yuv_plane_hvs), with plane_fidelity's images, pair table
        and semantics.  step: samples from an 8 x 8 DCT block to the next, 1 to 8 (8: the blocks do not overlap)."""
        cr, ct = (CeYuvImage * max(len(refs), 1))(), (CeYuvImage * max(len(tests), 1))()
        keep = []
        for arr, imgs in ((cr, refs), (ct, tests)):
            for i, img in enumerate(imgs):
                arr[i], k = img._c()
                keep.append(k)
        table = None if pair_ref is None else np.ascontiguousarray(pair_ref, dtype=np.uint32).reshape(-1)
        if table is not None and table.size != len(tests):
            raise CodecEvalError(CE_ERR_INVALID_ARG, f"pair_ref names {table.size} pairs for {len(tests)} tests")
        out = (CePlaneHvsScores * max(len(tests), 1))()
        self._check(lib().ce_yuv_plane_hvs(self._h, width, height, cr, len(refs), ct, len(tests),
                                           table.ctypes.data if table is not None else None, step, out))
        return [PlaneHvsScores.from_c(out[i]) for i in range(len(tests))]

    def plane_vif(self, refs: Sequence["YuvImage"], tests: Sequence["YuvImage"], width: int, height: int,
                  pair_ref: Optional[Sequence[int]] = None) -> List[PlaneVifScores]:
        """Pixel-domain VIF (VIFp) of Y'CbCr images plane by plane (ce_yuv_plane_vif), with plane_fidelity's images, pair table
        and semantics.  A plane needs 41 x 41 samples to run; luma must."""
        cr, ct = (CeYuvImage * max(len(refs), 1))(), (CeYuvImage * max(len(tests), 1))()
        keep = []
        for arr, imgs in ((cr, refs), (ct, tests)):
            for i, img in enumerate(imgs):
                arr[i], k = img._c()
                keep.append(k)
        table = None if pair_ref is None else np.ascontiguousarray(pair_ref, dtype=np.uint32).reshape(-1)
        if table is not None and table.size != len(tests):
            raise CodecEvalError(CE_ERR_INVALID_ARG, f"pair_ref names {table.size} pairs for {len(tests)} tests")
        out = (CePlaneVifScores * max(len(tests), 1))()
        self._check(lib().ce_yuv_plane_vif(self._h, width, height, cr, len(refs), ct, len(tests),
                                           table.ctypes.data if table is not None else None, out))
        return [PlaneVifScores.from_c(out[i]) for i in range(len(tests))]

    def plane_gmsd(self, refs: Sequence["YuvImage"], tests: Sequence["YuvImage"], width: int, height: int,
                   pair_ref: Optional[Sequence[int]] = None) -> List[PlaneGmsdScores]:
        """GMSD (gradient magnitude similarity deviation) and its mean of Y'CbCr images plane by plane (ce_yuv_plane_gmsd),
        with plane_fidelity's images, pair table and semantics.  Every plane of any size runs."""
        cr, ct = (CeYuvImage * max(len(refs), 1))(), (CeYuvImage * max(len(tests), 1))()
        keep = []
        for arr, imgs in ((cr, refs), (ct, tests)):
            for i, img in enumerate(imgs):
                arr[i], k = img._c()
                keep.append(k)
        table = None if pair_ref is None else np.ascontiguousarray(pair_ref, dtype=np.uint32).reshape(-1)
        if table is not None and table.size != len(tests):
            raise CodecEvalError(CE_ERR_INVALID_ARG, f"pair_ref names {table.size} pairs for {len(tests)} tests")
        out = (CePlaneGmsdScores * max(len(tests), 1))()
        self._check(lib().ce_yuv_plane_gmsd(self._h, width, height, cr, len(refs), ct, len(tests),
                                            table.ctypes.data if table is not None else None, out))
        return [PlaneGmsdScores.from_c(out[i]) for i in range(len(tests))]

    def delta_e_itp_map(self, reference, test, width: int, height: int, depth: int = 10, white_nits: float = 203.0, block: int = 1,
                        thresholds_q20=None, maps: bool = True):
        """Batch.delta_e_itp_maps for one pair of packed float32 RGB (ce_eval_pair_delta_e_itp_map): (uint32
        [1, ceil(h / block), ceil(w / block)] or None, uint64 [1, n] or None)."""
        r, t = _buf_f32(reference), _buf_f32(test)
        return _delta_e_itp_map(self, lambda m, n, thr, k, over: lib().ce_eval_pair_delta_e_itp_map(
            self._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, width, height, depth, white_nits, block, m, n, thr, k, over),
            1, width, height, block, thresholds_q20, maps)

    def batch_linear(self, width: int, height: int, max_refs: int, max_pairs: int) -> "Batch":
        """A Batch whose slabs hold packed float32 RGB in linear light (ce_batch_create_linear): loaded with float32 arrays
        through set_reference / set_test, or with tagged code values through set_reference_cicp / set_test_cicp."""
        return Batch(self, width, height, max_refs, max_pairs, linear=True)

    def cicp_to_linear(self, pixels, width: int, height: int, colour: "ColourDescription") -> np.ndarray:
        """One image of uint8 / uint16 RGB(A) code values read by `colour` -> [h, w, 3] float32 linear light with sRGB
        primaries, on the device (ce_cicp_to_linear)."""
        a = np.ascontiguousarray(pixels)
        out = np.empty((height, width, 3), np.float32)
        c = colour._c()
        self._check(lib().ce_cicp_to_linear(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c), width, height, out.ctypes.data,
                                            out.size))
        return out

    # the same leaves with alpha, blended in linear light over one background (include/ce_metrics.h: alpha in linear light)
    def _over_leaf(self, call, a, width, height, background, *mid):
        bg = _backgrounds_linear([background])
        out = np.empty((height, width, 3), np.float32)
        self._check(call(self._h, a.ctypes.data, a.nbytes, *mid, width, height, bg.ctypes.data, out.ctypes.data, out.size))
        return out

    def cicp_over_to_linear(self, pixels, width: int, height: int, colour: "ColourDescription", background) -> np.ndarray:
        """cicp_to_linear of an RGBA image, blended in linear light over `background` (three linear-light floats, sRGB
        primaries) on the device (ce_cicp_over_to_linear)."""
        a, c = np.ascontiguousarray(pixels), colour._c()
        return self._over_leaf(lib().ce_cicp_over_to_linear, a, width, height, background, _cicp_fmt(a), C.byref(c))

    def hlg_over_to_linear(self, pixels, width: int, height: int, description: "HlgDescription", background) -> np.ndarray:
        """hlg_to_linear of an RGBA image, blended in linear light over `background` (ce_hlg_over_to_linear)."""
        a, c = np.ascontiguousarray(pixels), description._c()
        return self._over_leaf(lib().ce_hlg_over_to_linear, a, width, height, background, _cicp_fmt(a), C.byref(c))

    def icc_over_to_linear(self, pixels, width: int, height: int, depth: int, profile: "IccProfile", background) -> np.ndarray:
        """icc_to_linear of an RGBA image, blended in linear light over `background` (ce_icc_over_to_linear)."""
        a = np.ascontiguousarray(pixels)
        return self._over_leaf(lib().ce_icc_over_to_linear, a, width, height, background, _cicp_fmt(a), depth, profile._h)

    def linear_over(self, pixels, width: int, height: int, background, premultiplied: bool = False) -> np.ndarray:
        """One (h, w, 4) float32 linear-light RGBA image, straight or premultiplied, over `background` (ce_linear_over)."""
        a = _rgba_f32(pixels)
        return self._over_leaf(lib().ce_linear_over, a, width, height, background, PIXEL_RGBA_F32, int(bool(premultiplied)))

    def icc_to_linear(self, pixels, width: int, height: int, depth: int, profile: "IccProfile") -> np.ndarray:
        """One image of uint8 / uint16 RGB(A) code values of `depth` bits read through a matrix/TRC profile -> [h, w, 3]
        float32 linear light with sRGB primaries, on the device (ce_icc_to_linear)."""
        a = np.ascontiguousarray(pixels)
        out = np.empty((height, width, 3), np.float32)
        self._check(lib().ce_icc_to_linear(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), depth, profile._h, width, height, out.ctypes.data,
                                           out.size))
        return out

    def icc_to_srgb(self, pixels, width: int, height: int, depth: int, profile: "IccProfile", depth_out: int = 8) -> np.ndarray:
        """The same image as sRGB code values: [h, w, 3] uint8 (depth_out = 8, ce_icc_to_srgb8) or uint16 of depth_out bits
        (10, 12 or 16, ce_icc_to_srgb16)."""
        a = np.ascontiguousarray(pixels)
        if depth_out == 8:
            out = np.empty((height, width, 3), np.uint8)
            self._check(lib().ce_icc_to_srgb8(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), depth, profile._h, width, height, out.ctypes.data,
                                              out.size))
        else:
            out = np.empty((height, width, 3), np.uint16)
            self._check(lib().ce_icc_to_srgb16(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), depth, profile._h, width, height, depth_out,
                                               out.ctypes.data, out.size))
        return out

    def hlg_to_linear(self, pixels, width: int, height: int, description: "HlgDescription") -> np.ndarray:
        """One image of uint8 / uint16 RGB(A) HLG code values read by `description` -> [h, w, 3] float32 display light with
        sRGB primaries, 1.0 = white_nits, on the device (ce_hlg_to_linear)."""
        a = np.ascontiguousarray(pixels)
        out = np.empty((height, width, 3), np.float32)
        c = description._c()
        self._check(lib().ce_hlg_to_linear(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c), width, height, out.ctypes.data,
                                           out.size))
        return out

    def gainmap_to_linear(self, pixels, width: int, height: int, colour: "ColourDescription", gain_map: "GainMap") -> np.ndarray:
        """One SDR base image of uint8 / uint16 RGB(A) code values read by `colour`, with `gain_map` applied -> [h, w, 3]
        float32 linear light with sRGB primaries, on the device (ce_gainmap_to_linear)."""
        a = np.ascontiguousarray(pixels)
        out = np.empty((height, width, 3), np.float32)
        c = colour._c()
        img, meta = gain_map._c()
        self._check(lib().ce_gainmap_to_linear(self._h, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c), C.byref(img), C.byref(meta), width,
                                               height, out.ctypes.data, out.size))
        return out

    def yuv_hlg_to_linear(self, image: "YuvImage", width: int, height: int, description: "HlgDescription") -> np.ndarray:
        """A decoder's Y'CbCr planes in HLG -> (height, width, 3) float32, in one kernel (ce_yuv_hlg_to_linear): yuv_to_rgb16
        at depth_out = description.depth followed by hlg_to_linear, bit for bit."""
        c, _keep = image._c()
        d = description._c()
        out = np.empty((height, width, 3), np.float32)
        self._check(lib().ce_yuv_hlg_to_linear(self._h, C.byref(c), C.byref(d), width, height, out.ctypes.data, out.size))
        return out

    def batch_deep(self, width: int, height: int, max_refs: int, max_pairs: int, ref_depth: int, test_depth: int) -> "Batch":
        """A Batch whose slabs hold uint16 samples of the given depths (8, 10, 12 or 16 bits per side)."""
        return Batch(self, width, height, max_refs, max_pairs, depths=(ref_depth, test_depth))

    def copy_device(self, dst: int, src: int, nbytes: int):
        """`nbytes` from one device address to another on the context's stream (for callers that move images between the
        slabs Batch.reference_slab / test_slab expose): ordered like a kernel of this context."""
        rc = lib().hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3, C.c_void_p(self.stream))  # 3: device to device
        if rc != 0:
            raise MetricCalculation(CE_ERR_BACKEND, f"hipMemcpyAsync failed with {rc}")

    def host_buffer(self, nbytes: int) -> np.ndarray:
        """`nbytes` of page-locked host memory as a flat uint8 array (ce_host_alloc; freed when the array and every view of
        it are gone): images placed here are uploaded by DMA straight from the buffer, overlapped with the kernels."""
        p = C.c_void_p()
        self._check(lib().ce_host_alloc(self._h, nbytes, C.byref(p)))
        return np.frombuffer(_pinned_block(p.value, nbytes), dtype=np.uint8)

    def eval_batch(self, pairs, config: MetricConfig,
                   intensity_target: float = DEFAULT_INTENSITY_TARGET, test_tables: Optional[Sequence] = None) -> List[CeScores]:
        """pairs: (reference, test, width, height) tuples, or a PairList built from them once (a caller that scores the same
        buffers again and again - a decoder writing into fixed page-locked images - then pays the descriptor marshalling
        once, as a compiled caller of ce_eval_batch does).  The (codec x quality) grid of session.rs:375-376.
        test_tables: optional per-pair ColorTable (or None) applied to the distorted image on the device."""
        pl = pairs if isinstance(pairs, PairList) else PairList(pairs)
        n = pl.n
        out = (CeScores * n)()
        if test_tables is not None:
            luts = (C.c_void_p * n)(*[(t._h if t is not None else None) for t in test_tables])
            self._check(lib().ce_eval_batch_lut(self._h, n, pl.descs, luts, config.mask, config.flags, intensity_target, out))
        else:
            self._check(lib().ce_eval_batch(self._h, n, pl.descs, config.mask, config.flags, intensity_target, out))
        return list(out)

    # -- measurement hooks
    def prof_enable(self, on=True, serial: bool = True):
        """Per-kernel HIP-event timing.  serial=True: one kernel at a time on the context's stream (solo
        times); serial=False: keep the batch's multi-stream schedule (times as rocprofv3 sees them)."""
        self._check(lib().ce_prof_enable(self._h, 0 if not on else (1 if serial else 2)))

    def prof_filter(self, substring: str = ""):
        """Only kernels whose name contains `substring` get events ("" = all, "=name" = exactly that kernel)."""
        self._check(lib().ce_prof_filter(self._h, substring.encode()))

    def prof_reset(self):
        self._check(lib().ce_prof_reset(self._h))

    def prof_stats(self) -> dict:
        L = lib()
        out = {}
        for i in range(L.ce_prof_count(self._h)):
            name, n, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self._check(L.ce_prof_get(self._h, i, C.byref(name), C.byref(n), C.byref(ms)))
            out[name.value.decode()] = (int(n.value), float(ms.value))
        return out

    def timer_start(self):
        self._check(lib().ce_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_double()
        self._check(lib().ce_timer_stop(self._h, C.byref(ms)))
        return ms.value


class ColorTable:
    """ICC -> sRGB as a complete colour table on the device (ce_lut_*): `table[r, g, b] = transform(r, g, b)`, uint8,
    shape (256, 256, 256, 3) - the host CMS evaluated once on the identity colour cube (`identity_cube()`), which
    reproduces an 8-bit RGB -> 8-bit RGB transform such as the reference's (icc.rs:69-103) bit for bit."""

    def __init__(self, ctx: "Context", table):
        t = np.ascontiguousarray(np.asarray(table, dtype=np.uint8)).reshape(-1)
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx._check(lib().ce_lut_create(ctx._h, t.ctypes.data, t.size, C.byref(self._h)))

    @staticmethod
    def identity_cube() -> np.ndarray:
        """All 2^24 colours as an (2^24, 3) uint8 array in table order: feed it to the CMS, pass the result to ColorTable."""
        v = np.arange(1 << 24, dtype=np.uint32)
        return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8)

    def close(self):
        if self._h and self.ctx._h:
            lib().ce_lut_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IccProfile:
    """A matrix/TRC ICC profile applied on the device (ce_icc_*): three colorants and three tone curves, parsed by the
    library itself - no CMS.  Any other profile (LUT-based, Gray, CMYK, malformed) raises CodecEvalError with the reason;
    `icc_describe(profile).kind` tells which without raising.  Close it after the last batch that was given it has been
    collected."""

    def __init__(self, ctx: "Context", profile: bytes):
        b = bytes(profile)
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx._check(lib().ce_icc_create(ctx._h, b, len(b), C.byref(self._h)))

    def close(self):
        if self._h and self.ctx._h:
            lib().ce_icc_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IccLutProfile(IccProfile):
    """A LUT-based ICC profile applied on the device (ce_icc_lut_create): an A2B tag of type mAB, mft2 or mft1, evaluated from
    the profile itself - no CMS, no 2^24-entry table.  Accepted wherever an IccProfile is.  `intent` 0, 1 or 2 chooses A2B0 /
    A2B1 / A2B2 (A2B0 where the other is absent); `interpolation` is ICC_CLUT_TRILINEAR or ICC_CLUT_TETRAHEDRAL.  Any other
    profile raises CodecEvalError with the reason; `icc_lut_describe(profile).kind` tells which without raising."""

    def __init__(self, ctx: "Context", profile: bytes, intent: int = 0, interpolation: int = ICC_CLUT_TRILINEAR):
        b = bytes(profile)
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx._check(lib().ce_icc_lut_create(ctx._h, b, len(b), intent, interpolation, C.byref(self._h)))


class Batch:
    """HBM-resident grid of (reference, test) pairs of one shape (ce_batch_*)."""

    def __init__(self, ctx: Context, width: int, height: int, max_refs: int, max_pairs: int,
                 depths: Optional[Tuple[int, int]] = None, linear: bool = False):
        """depths=(reference depth, test depth): a deep batch (ce_batch_create_deep) - set_reference / set_test then also
        take uint16 arrays ([h, w, 3] or flat RGB, [h, w, 4] RGBA) of that side's depth.  linear=True: a linear batch
        (ce_batch_create_linear) - set_reference / set_test take float32 arrays, set_*_cicp tagged code values."""
        if linear and depths is not None:
            raise ValueError("a batch is deep or linear, not both")
        self.linear = linear
        self.ctx, self.width, self.height = ctx, width, height
        self.max_refs, self.max_pairs = max_refs, max_pairs
        self.depths = tuple(depths) if depths is not None else None
        self._pair_ref = [0] * max_pairs  # the pair -> reference bindings, as the library holds them
        self._h = C.c_void_p()
        if linear:
            ctx._check(lib().ce_batch_create_linear(ctx._h, width, height, max_refs, max_pairs, C.byref(self._h)))
        elif self.depths is None:
            ctx._check(lib().ce_batch_create(ctx._h, width, height, max_refs, max_pairs, C.byref(self._h)))
        else:
            ctx._check(lib().ce_batch_create_deep(ctx._h, width, height, max_refs, max_pairs, self.depths[0], self.depths[1],
                                                  C.byref(self._h)))

    @staticmethod
    def _deep_fmt(a: np.ndarray) -> int:
        return PIXEL_RGBA16 if a.ndim == 3 and a.shape[-1] == 4 else PIXEL_RGB16

    def close(self):
        if self._h and self.ctx._h:
            lib().ce_batch_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_reference(self, ref_index: int, rgb):
        if np.asarray(rgb).dtype == np.float32:
            return self.set_reference_fmt(ref_index, rgb, PIXEL_RGB_F32)
        if np.asarray(rgb).dtype == np.uint16:
            return self.set_reference_fmt(ref_index, rgb, self._deep_fmt(np.asarray(rgb)))
        r = _buf(rgb)
        self.ctx._check(lib().ce_batch_set_reference(self._h, ref_index, r.ctypes.data, r.size))

    def set_test(self, pair_index: int, ref_index: int, rgb):
        if np.asarray(rgb).dtype == np.float32:
            return self.set_test_fmt(pair_index, ref_index, rgb, PIXEL_RGB_F32)
        if np.asarray(rgb).dtype == np.uint16:
            return self.set_test_fmt(pair_index, ref_index, rgb, self._deep_fmt(np.asarray(rgb)))
        t = _buf(rgb)
        self.ctx._check(lib().ce_batch_set_test(self._h, pair_index, ref_index, t.ctypes.data, t.size))
        self._pair_ref[pair_index] = ref_index

    # decoded-image ingest: pixels as a decoder hands them over, converted to RGB8 on the device
    def set_reference_fmt(self, ref_index: int, pixels, fmt: int):
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_reference_fmt(self._h, ref_index, a.ctypes.data, a.nbytes, fmt))

    def set_test_fmt(self, pair_index: int, ref_index: int, pixels, fmt: int):
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_test_fmt(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, fmt))
        self._pair_ref[pair_index] = ref_index

    # tagged code values (H.273 primaries / transfer) -> linear light on the device, into a slot of a linear batch
    def set_reference_cicp(self, ref_index: int, pixels, colour: "ColourDescription"):
        a, c = np.ascontiguousarray(pixels), colour._c()
        self.ctx._check(lib().ce_batch_set_reference_cicp(self._h, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c)))

    def set_test_cicp(self, pair_index: int, ref_index: int, pixels, colour: "ColourDescription"):
        a, c = np.ascontiguousarray(pixels), colour._c()
        self.ctx._check(lib().ce_batch_set_test_cicp(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c)))
        self._pair_ref[pair_index] = ref_index

    # a decoder's Y'CbCr planes, host or device: upsampled and converted on the device, straight into the slot
    def set_reference_yuv(self, ref_index: int, image: "YuvImage"):
        c, _keep = image._c()
        self.ctx._check(lib().ce_batch_set_reference_yuv(self._h, ref_index, C.byref(c)))

    def set_test_yuv(self, pair_index: int, ref_index: int, image: "YuvImage"):
        c, _keep = image._c()
        self.ctx._check(lib().ce_batch_set_test_yuv(self._h, pair_index, ref_index, C.byref(c)))
        self._pair_ref[pair_index] = ref_index

    # a framework's strided tensors, host or device: read through their strides and converted on the device, all images of
    # the tensor in consecutive slots; a device tensor is read in place, behind what the context's stream holds at the call
    def _tensor_c(self, image: "TensorImage") -> CeTensorImage:
        if (image.width, image.height) != (self.width, self.height):
            raise ValueError(f"a tensor of {image.width} x {image.height} for a batch of {self.width} x {self.height}")
        return image._c()

    def set_reference_tensor(self, first_ref: int, image: "TensorImage"):
        """Images 0 .. image.count - 1 into reference slots first_ref .. (ce_batch_set_reference_tensor)."""
        c = self._tensor_c(image)
        self.ctx._check(lib().ce_batch_set_reference_tensor(self._h, first_ref, image.count, C.byref(c)))

    def set_test_tensor(self, first_pair: int, ref_indices: Sequence[int], image: "TensorImage"):
        """Images 0 .. image.count - 1 into test slots first_pair .., pair first_pair + n bound to reference ref_indices[n]
        (ce_batch_set_test_tensor)."""
        c = self._tensor_c(image)
        refs = np.ascontiguousarray(ref_indices, dtype=np.uint32)
        if refs.shape != (image.count,):
            raise ValueError("set_test_tensor takes one reference index per image of the tensor")
        self.ctx._check(lib().ce_batch_set_test_tensor(self._h, first_pair, refs.ctypes.data, image.count, C.byref(c)))
        for k, r in enumerate(refs):
            self._pair_ref[first_pair + k] = int(r)

    # code values with a matrix/TRC ICC profile, applied by the library itself, into a slot of any batch
    def set_reference_icc(self, ref_index: int, pixels, depth: int, profile: "IccProfile"):
        """uint8 / uint16 RGB(A) code values of `depth` bits read through a matrix/TRC profile, into a reference slot of any
        batch: linear light in a linear batch, sRGB code values of the slot's depth otherwise (ce_batch_set_reference_icc)."""
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_reference_icc(self._h, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), depth, profile._h))

    def set_test_icc(self, pair_index: int, ref_index: int, pixels, depth: int, profile: "IccProfile"):
        """The same for the test image of pair `pair_index`, bound to reference `ref_index` (ce_batch_set_test_icc)."""
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_test_icc(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), depth, profile._h))
        self._pair_ref[pair_index] = ref_index

    # the same planes with a colour description -> linear light in one kernel, into a slot of a linear batch
    def set_reference_yuv_cicp(self, ref_index: int, image: "YuvImage", colour: "ColourDescription"):
        c, _keep = image._c()
        col = colour._c()
        self.ctx._check(lib().ce_batch_set_reference_yuv_cicp(self._h, ref_index, C.byref(c), C.byref(col)))

    def set_test_yuv_cicp(self, pair_index: int, ref_index: int, image: "YuvImage", colour: "ColourDescription"):
        c, _keep = image._c()
        col = colour._c()
        self.ctx._check(lib().ce_batch_set_test_yuv_cicp(self._h, pair_index, ref_index, C.byref(c), C.byref(col)))
        self._pair_ref[pair_index] = ref_index

    # the same planes with an ICC profile of either flavour, in one kernel, into a slot of any batch
    def set_reference_yuv_icc(self, ref_index: int, image: "YuvImage", rgb_depth: int, profile: "IccProfile"):
        """A decoder's Y'CbCr planes, host or device, read through `profile` into a reference slot of any batch: linear light in
        a linear batch, sRGB code values of the slot's depth otherwise (ce_batch_set_reference_yuv_icc).  rgb_depth (8, 10, 12 or
        16, not under the planes' depth) is the integer RGB grid between the colour matrix and the profile."""
        c, _keep = image._c()
        self.ctx._check(lib().ce_batch_set_reference_yuv_icc(self._h, ref_index, C.byref(c), rgb_depth, profile._h if profile is not None else None))

    def set_test_yuv_icc(self, pair_index: int, ref_index: int, image: "YuvImage", rgb_depth: int, profile: "IccProfile"):
        """The same for the test image of pair `pair_index`, bound to reference `ref_index` (ce_batch_set_test_yuv_icc)."""
        c, _keep = image._c()
        self.ctx._check(lib().ce_batch_set_test_yuv_icc(self._h, pair_index, ref_index, C.byref(c), rgb_depth, profile._h if profile is not None else None))
        self._pair_ref[pair_index] = ref_index

    # BT.2100 HLG code values, and planes, -> display light on the device, into a slot of a linear batch
    def set_reference_hlg(self, ref_index: int, pixels, description: "HlgDescription"):
        a, c = np.ascontiguousarray(pixels), description._c()
        self.ctx._check(lib().ce_batch_set_reference_hlg(self._h, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c)))

    def set_test_hlg(self, pair_index: int, ref_index: int, pixels, description: "HlgDescription"):
        a, c = np.ascontiguousarray(pixels), description._c()
        self.ctx._check(lib().ce_batch_set_test_hlg(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c)))
        self._pair_ref[pair_index] = ref_index

    def set_reference_yuv_hlg(self, ref_index: int, image: "YuvImage", description: "HlgDescription"):
        c, _keep = image._c()
        d = description._c()
        self.ctx._check(lib().ce_batch_set_reference_yuv_hlg(self._h, ref_index, C.byref(c), C.byref(d)))

    def set_test_yuv_hlg(self, pair_index: int, ref_index: int, image: "YuvImage", description: "HlgDescription"):
        c, _keep = image._c()
        d = description._c()
        self.ctx._check(lib().ce_batch_set_test_yuv_hlg(self._h, pair_index, ref_index, C.byref(c), C.byref(d)))
        self._pair_ref[pair_index] = ref_index

    # an SDR base image with a gain map -> the HDR rendition on the device, into a slot of a linear batch
    def set_reference_gainmap(self, ref_index: int, pixels, colour: "ColourDescription", gain_map: "GainMap"):
        a, c = np.ascontiguousarray(pixels), colour._c()
        img, meta = gain_map._c()
        self.ctx._check(lib().ce_batch_set_reference_gainmap(self._h, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c), C.byref(img),
                                                             C.byref(meta)))

    def set_test_gainmap(self, pair_index: int, ref_index: int, pixels, colour: "ColourDescription", gain_map: "GainMap"):
        a, c = np.ascontiguousarray(pixels), colour._c()
        img, meta = gain_map._c()
        self.ctx._check(lib().ce_batch_set_test_gainmap(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, _cicp_fmt(a), C.byref(c),
                                                        C.byref(img), C.byref(meta)))
        self._pair_ref[pair_index] = ref_index

    # a transparent image composited over solid colours on the device: one upload fills len(backgrounds) consecutive slots
    def set_reference_over(self, first_ref: int, pixels, fmt: int, backgrounds):
        a, bg = np.ascontiguousarray(pixels), _backgrounds(backgrounds)
        self.ctx._check(lib().ce_batch_set_reference_over(self._h, first_ref, a.ctypes.data, a.nbytes, fmt, len(bg), bg.ctypes.data))

    def set_test_over(self, first_pair: int, ref_indices: Sequence[int], pixels, fmt: int, backgrounds):
        a, bg = np.ascontiguousarray(pixels), _backgrounds(backgrounds)
        refs = np.ascontiguousarray(ref_indices, dtype=np.uint32)
        if refs.shape != (len(bg),):
            raise ValueError("set_test_over takes one reference index per background")
        self.ctx._check(lib().ce_batch_set_test_over(self._h, first_pair, refs.ctypes.data, a.ctypes.data, a.nbytes, fmt, len(bg), bg.ctypes.data))
        for k, r in enumerate(refs):
            self._pair_ref[first_pair + k] = int(r)

    # an image with alpha turned into linear light and blended there over solid colours (include/ce_metrics.h: alpha in linear
    # light): one upload fills len(backgrounds) consecutive slots of a linear batch; backgrounds are rows of three linear floats
    def _set_over_linear(self, name, test, first, ref_indices, a, backgrounds, *mid):
        bg = _backgrounds_linear(backgrounds)
        if not test:
            self.ctx._check(getattr(lib(), "ce_batch_set_reference_" + name)(self._h, first, a.ctypes.data, a.nbytes, *mid, len(bg), bg.ctypes.data))
            return
        refs = np.ascontiguousarray(ref_indices, dtype=np.uint32)
        if refs.shape != (len(bg),):
            raise ValueError("set_test_*_over takes one reference index per background")
        self.ctx._check(getattr(lib(), "ce_batch_set_test_" + name)(self._h, first, refs.ctypes.data, a.ctypes.data, a.nbytes, *mid, len(bg),
                                                                    bg.ctypes.data))
        for k, r in enumerate(refs):
            self._pair_ref[first + k] = int(r)

    def set_reference_cicp_over(self, first_ref: int, pixels, colour: "ColourDescription", backgrounds):
        a, c = np.ascontiguousarray(pixels), colour._c()
        self._set_over_linear("cicp_over", False, first_ref, None, a, backgrounds, _cicp_fmt(a), C.byref(c))

    def set_test_cicp_over(self, first_pair: int, ref_indices: Sequence[int], pixels, colour: "ColourDescription", backgrounds):
        a, c = np.ascontiguousarray(pixels), colour._c()
        self._set_over_linear("cicp_over", True, first_pair, ref_indices, a, backgrounds, _cicp_fmt(a), C.byref(c))

    def set_reference_hlg_over(self, first_ref: int, pixels, description: "HlgDescription", backgrounds):
        a, c = np.ascontiguousarray(pixels), description._c()
        self._set_over_linear("hlg_over", False, first_ref, None, a, backgrounds, _cicp_fmt(a), C.byref(c))

    def set_test_hlg_over(self, first_pair: int, ref_indices: Sequence[int], pixels, description: "HlgDescription", backgrounds):
        a, c = np.ascontiguousarray(pixels), description._c()
        self._set_over_linear("hlg_over", True, first_pair, ref_indices, a, backgrounds, _cicp_fmt(a), C.byref(c))

    def set_reference_icc_over(self, first_ref: int, pixels, depth: int, profile: "IccProfile", backgrounds):
        a = np.ascontiguousarray(pixels)
        self._set_over_linear("icc_over", False, first_ref, None, a, backgrounds, _cicp_fmt(a), depth, profile._h)

    def set_test_icc_over(self, first_pair: int, ref_indices: Sequence[int], pixels, depth: int, profile: "IccProfile", backgrounds):
        a = np.ascontiguousarray(pixels)
        self._set_over_linear("icc_over", True, first_pair, ref_indices, a, backgrounds, _cicp_fmt(a), depth, profile._h)

    def set_reference_linear_over(self, first_ref: int, pixels, backgrounds, premultiplied: bool = False):
        self._set_over_linear("linear_over", False, first_ref, None, _rgba_f32(pixels), backgrounds, PIXEL_RGBA_F32, int(bool(premultiplied)))

    def set_test_linear_over(self, first_pair: int, ref_indices: Sequence[int], pixels, backgrounds, premultiplied: bool = False):
        self._set_over_linear("linear_over", True, first_pair, ref_indices, _rgba_f32(pixels), backgrounds, PIXEL_RGBA_F32, int(bool(premultiplied)))

    # ... and through a colour table (ICC -> sRGB on the device)
    def set_reference_lut(self, ref_index: int, pixels, fmt: int, table: Optional["ColorTable"]):
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_reference_lut(self._h, ref_index, a.ctypes.data, a.nbytes, fmt, table._h if table else None))

    def set_test_lut(self, pair_index: int, ref_index: int, pixels, fmt: int, table: Optional["ColorTable"]):
        a = np.ascontiguousarray(pixels)
        self.ctx._check(lib().ce_batch_set_test_lut(self._h, pair_index, ref_index, a.ctypes.data, a.nbytes, fmt, table._h if table else None))
        self._pair_ref[pair_index] = ref_index

    def bind_pair(self, pair_index: int, ref_index: int):
        self.ctx._check(lib().ce_batch_bind_pair(self._h, pair_index, ref_index))
        self._pair_ref[pair_index] = ref_index

    def pair_reference(self, pair_index: int) -> int:
        """The reference pair `pair_index` is bound to (0 until a set_test* / bind_pair names another)."""
        return self._pair_ref[pair_index]

    @property
    def reference_slab(self) -> int:
        return int(lib().ce_batch_reference_slab(self._h))

    @property
    def test_slab(self) -> int:
        return int(lib().ce_batch_test_slab(self._h))

    def references_changed(self):
        """References were written through a kept `reference_slab` address: the next launch rebuilds what the metrics
        derive from them (reading `reference_slab` again says the same)."""
        self.ctx._check(lib().ce_batch_references_changed(self._h))

    def ref_stats(self):
        """(ssimulacra2, dssim, butteraugli): launches so far that (re)built that metric's reference-side state."""
        out = (_u32 * 3)()
        self.ctx._check(lib().ce_batch_ref_stats(self._h, C.byref(out)))
        return tuple(out)

    def run(self, n_pairs: int, config: MetricConfig, intensity_target: float = DEFAULT_INTENSITY_TARGET,
            butteraugli_diffmap: bool = False, ssimulacra2_maps: bool = False) -> List[CeScores]:
        """butteraugli_diffmap=True: also keep every pair's Butteraugli diffmap for butteraugli_diffmaps();
        ssimulacra2_maps=True: every pair's SSIMULACRA2 error maps for ssimulacra2_maps()."""
        out = (CeScores * n_pairs)()
        flags = config.flags | (FLAG_BUTTERAUGLI_DIFFMAP if butteraugli_diffmap else 0) | (FLAG_SSIMULACRA2_MAPS if ssimulacra2_maps else 0)
        self.ctx._check(lib().ce_batch_run(self._h, n_pairs, config.mask, flags, intensity_target, out))
        return list(out)

    def launch(self, n_pairs: int, config: MetricConfig, intensity_target: float = DEFAULT_INTENSITY_TARGET,
               butteraugli_diffmap: bool = False, ssimulacra2_maps: bool = False):
        flags = config.flags | (FLAG_BUTTERAUGLI_DIFFMAP if butteraugli_diffmap else 0) | (FLAG_SSIMULACRA2_MAPS if ssimulacra2_maps else 0)
        self.ctx._check(lib().ce_batch_launch(self._h, n_pairs, config.mask, flags, intensity_target))

    def collect(self, n_pairs: int) -> List[CeScores]:
        out = (CeScores * n_pairs)()
        self.ctx._check(lib().ce_batch_collect(self._h, n_pairs, out))
        return list(out)

    def ms_ssim(self, n_pairs: int, levels: int = 5) -> List[MsSsim]:
        """SSIM (levels = 1) and MS-SSIM (5) of pairs [0, n_pairs) of an RGB8 or equal-depth deep batch on the encoded sample
        values (ce_batch_msssim); returns once the scores are on the host.  Scores and maps of a launch are untouched."""
        out = (CeMsssimScores * max(n_pairs, 1))()
        self.ctx._check(lib().ce_batch_msssim(self._h, n_pairs, levels, out))
        return [MsSsim.from_c(out[i]) for i in range(n_pairs)]

    def ciede2000(self, n_pairs: int, thresholds_q20=None) -> List[Ciede2000]:
        """CIEDE2000 of pairs [0, n_pairs) of an RGB8 or deep batch read as sRGB (ce_batch_ciede2000); returns once the scores
        are on the host.  thresholds_q20: up to eight values in units of 2^-20 whose exceedance counts come back in n_above.
        Scores and maps of a launch are untouched."""
        out = (CeCiede2000Scores * max(n_pairs, 1))()
        thr = _thresholds_q20(thresholds_q20)
        self.ctx._check(lib().ce_batch_ciede2000(self._h, n_pairs, thr.ctypes.data if thr.size else None, thr.size, out))
        return [Ciede2000.from_c(out[i]) for i in range(n_pairs)]

    def ciede2000_maps(self, first: int, count: int, what="de", block: int = 1, thresholds_q20=None, maps: bool = True):
        """Where pairs [first, first + count) of an RGB8 or deep batch read as sRGB differ, and in which direction of colour space
        (ce_batch_ciede2000_map): per pixel one of four values in units of 2^-20 (CIEDE2000_Q20 is 1.0) - with what="de" the
        Delta E 2000, the very integer ciede2000() sums; with "dl", "dc" or "dh" the magnitude of its lightness, chroma or hue
        term, which may exceed the Delta E - as a uint32 [count, h, w] array, or at block = 2 .. 64 the maximum of each block x
        block cell, [count, ceil(h / block), ceil(w / block)]; and for up to 8 `thresholds_q20` how many pixels of each pair
        exceed each, uint64 [count, n].  maps=False: counts only (None for the maps); thresholds_q20=None: maps only.  What
        launch() left to collect and ciede2000()'s results are untouched."""
        return _ciede2000_map(self.ctx, lambda wh, m, n, thr, k, over: lib().ce_batch_ciede2000_map(
            self._h, first, count, wh, block, m, n, thr, k, over), count, self.width, self.height, what, block, thresholds_q20, maps)

    def ms_ssim_maps(self, first: int, count: int, levels: int = 5, level: int = 0, what: str = "ssim", block: int = 1, thresholds_q32=None,
                     maps: bool = True):
        """Where pairs [first, first + count) of an RGB8 or equal-depth deep batch differ at `level` of the SSIM (levels = 1) or
        MS-SSIM (5) pyramid (ce_batch_msssim_map): at every valid position of R, G and B the dissimilarity 2^32 - q in units of
        2^-32 (MSSSIM_Q32 is an SSIM of 1.0), q the very integer ms_ssim() sums - of SSIM with what="ssim", of the
        contrast-structure term with "cs" - saturated to [0, 2^32 - 1], as a uint32 [count, 3, vh, vw] array, or at block = 2 ..
        64 the maximum of each block x block cell, [count, 3, ceil(vh / block), ceil(vw / block)]; and for up to 8
        `thresholds_q32` how many positions of each pair and channel exceed each, uint64 [count, 3, n].  maps=False: counts only
        (None for the maps); thresholds_q32=None: maps only.  What launch() left to collect and ms_ssim()'s results are untouched."""
        return _msssim_map(self.ctx, lambda wh, m, n, thr, k, over: lib().ce_batch_msssim_map(
            self._h, first, count, levels, level, wh, block, m, n, thr, k, over), count, self.width, self.height, levels, level, what, block,
            thresholds_q32, maps)

    def hdr_fidelity(self, n_pairs: int, depth: int = 10, white_nits: float = 203.0) -> List[HdrFidelity]:
        """PQ-PSNR and BT.2124 Delta E ITP of pairs [0, n_pairs) of a linear batch (ce_batch_hdr_fidelity); returns once the
        scores are on the host.  What launch() left to collect is untouched."""
        out = (CeHdrScores * max(n_pairs, 1))()
        self.ctx._check(lib().ce_batch_hdr_fidelity(self._h, n_pairs, depth, white_nits, out))
        return [HdrFidelity.from_c(out[i]) for i in range(n_pairs)]

    def delta_e_itp_maps(self, first: int, count: int, depth: int = 10, white_nits: float = 203.0, block: int = 1, thresholds_q20=None,
                         maps: bool = True):
        """Where pairs [first, first + count) of a linear batch differ (ce_batch_delta_e_itp_map): every pixel's BT.2124
        Delta E ITP in units of 2^-20 (DELTA_E_ITP_Q20 is 1.0), saturated at 2^32 - 1, as a uint32 [count, h, w] array, or at
        block = 2 .. 64 the maximum of each block x block cell, [count, ceil(h / block), ceil(w / block)]; and for up to 8
        `thresholds_q20` how many pixels of each pair exceed each, uint64 [count, n].  maps=False: counts only (None for the
        maps); thresholds_q20=None: maps only.  What launch() left to collect is untouched."""
        return _delta_e_itp_map(self.ctx, lambda m, n, thr, k, over: lib().ce_batch_delta_e_itp_map(
            self._h, first, count, depth, white_nits, block, m, n, thr, k, over), count, self.width, self.height, block, thresholds_q20, maps)

    def butteraugli_pnorm3(self, n_pairs: int) -> np.ndarray:
        out = np.zeros(n_pairs, np.float64)
        self.ctx._check(lib().ce_batch_butteraugli_pnorm3(self._h, n_pairs, out.ctypes.data_as(_dp)))
        return out

    def butteraugli_diffmaps(self, first: int, count: int, block: int = 1) -> np.ndarray:
        """Diffmaps of pairs [first, first + count) of the last run / launch with butteraugli_diffmap=True, as a
        [count, ceil(h / block), ceil(w / block)] float32 array: block = 1 is the full map, a power of two up to 64 the
        maximum over each block x block cell."""
        return _read_diffmaps(self.ctx, lib().ce_batch_butteraugli_diffmap, self._h, self.width, self.height, first, count, block)

    def dssim_ssim_maps(self, level: int, first: int, count: int, block: int = 1):
        """DSSIM's SsimMap at `level` of pairs [first, first + count) of the last run / launch with DSSIM:
        (maps, float32 [count, ceil(h_l / block), ceil(w_l / block)], ssim, float64 [count]).  block = 1 is the full map, a
        power of two up to 64 the minimum over each block x block cell."""
        return _read_ssim_maps(self.ctx, lib().ce_batch_dssim_ssim_maps, self._h, self.width, self.height, level, first, count, block)

    def ssimulacra2_maps(self, scale: int, channel: int, kind: int, first: int, count: int, block: int = 1, maps: bool = True):
        """SSIMULACRA2's map `kind` (SSIM2_MAP_*) of XYB `channel` at `scale` for pairs [first, first + count) of the last
        run / launch: (maps, float32 [count, ceil(h_s / block), ceil(w_s / block)], norms, float64 [count, 2] - the map's
        mean and 4-norm as the score pooled them).  block = 1 is the full map, a power of two up to 64 the maximum over each
        block x block cell.  The maps need ssimulacra2_maps=True at launch; maps=False reads the norms alone (maps None),
        which every launch with SSIMULACRA2 leaves."""
        return _read_ssim2_maps(self.ctx, lib().ce_batch_ssimulacra2_maps, self._h, self.width, self.height, scale, channel, kind,
                                first, count, block, maps)

    def image_heuristics(self, first: int, count: int, tests: bool = False) -> List[ImageHeuristics]:
        """compute_heuristics of references (tests=True: test images) [first, first + count) as they sit in the batch,
        after every set_* / bind_pair so far; the last run's scores and maps stay as they are."""
        out = (CeImageHeuristics * max(count, 1))()
        self.ctx._check(lib().ce_batch_image_heuristics(self._h, BATCH_TESTS if tests else BATCH_REFERENCES, first, count, out))
        return [ImageHeuristics.from_c(out[i]) for i in range(count)]

    def resample_into(self, dst: "Batch", first: int, count: int, tests: bool = False, filter: int = RESAMPLE_LANCZOS3):
        """References (tests=True: test images) [first, first + count) of this batch resampled to `dst`'s shape into the
        same indices of `dst`, a batch of the same context and the same kind - RGB8 into RGB8 by the fixed-point resampler,
        linear into linear by the float one (ce_batch_resample): on the device, behind this batch's
        uploads and ahead of dst's next launch; no scores or maps of either batch change."""
        self.ctx._check(lib().ce_batch_resample(self._h, dst._h, BATCH_TESTS if tests else BATCH_REFERENCES, first, count, filter))

    def resample_pairs_into(self, dst: "Batch", n_refs: int, n_pairs: int, filter: int = RESAMPLE_LANCZOS3):
        """References [0, n_refs) and tests [0, n_pairs) resampled into `dst` together with the pairs' reference
        bindings (ce_batch_resample_pairs): `dst.run(n_pairs, ...)` follows directly."""
        self.ctx._check(lib().ce_batch_resample_pairs(self._h, dst._h, n_refs, n_pairs, filter))
        dst._pair_ref[:n_pairs] = self._pair_ref[:n_pairs]

    # -- test hooks
    def debug_limit_scales(self, n: int):
        self.ctx._check(lib().ce_debug_ssim2_limit_scales(self._h, n))

    def debug_planes(self, scale: int, which: int, channel: int = 0) -> np.ndarray:
        nplanes = 5 if which == 4 else 3
        buf = np.empty(nplanes * self.width * self.height, np.float32)
        w, h = C.c_uint32(), C.c_uint32()
        self.ctx._check(lib().ce_debug_ssim2_planes(self._h, scale, which, channel, buf.ctypes.data, buf.size,
                                                     C.byref(w), C.byref(h)))
        return buf[: nplanes * w.value * h.value].reshape(nplanes, h.value, w.value).copy()

    def debug_dssim_walk_rows(self, rows: int):
        """Force the rows a wave of DSSIM's streaming kernels walks in later runs (0 = automatic, else 2, 4, .. 64)."""
        self.ctx._check(lib().ce_debug_dssim_walk_rows(self._h, rows))

    def debug_averages(self, pair_index: int) -> np.ndarray:
        avg = np.zeros((6, 3, 6), np.float64)
        ns = C.c_int()
        self.ctx._check(lib().ce_debug_ssim2_averages(self._h, pair_index, avg.ctypes.data_as(_dp), C.byref(ns)))
        return avg[: ns.value].copy()


class ReferenceHandle:
    """Ssimulacra2Reference::{new, compare} (crates/codec-iter/src/eval.rs:138-149, 83-89)."""

    def __init__(self, ctx: Context, reference, width: int, height: int, xyb_roundtrip: bool = False,
                 butteraugli_diffmap: bool = False, ssimulacra2_maps: bool = False):
        self.ctx, self.width, self.height = ctx, width, height
        r = _buf(reference)
        self._h = C.c_void_p()
        flags = ((FLAG_XYB_ROUNDTRIP if xyb_roundtrip else 0) | (FLAG_BUTTERAUGLI_DIFFMAP if butteraugli_diffmap else 0) |
                 (FLAG_SSIMULACRA2_MAPS if ssimulacra2_maps else 0))
        ctx._check(lib().ce_ref_create(ctx._h, r.ctypes.data, r.size, width, height, flags, C.byref(self._h)))

    def compare(self, test, config: MetricConfig = None, intensity_target: float = DEFAULT_INTENSITY_TARGET) -> MetricResult:
        config = config or MetricConfig.ssimulacra2_only()
        t = _buf(test)
        s = CeScores()
        self.ctx._check(lib().ce_ref_compare(self._h, t.ctypes.data, t.size, config.mask, intensity_target, C.byref(s)))
        return MetricResult.from_c(s)

    def compare_many(self, tests, config: MetricConfig = None, intensity_target: float = DEFAULT_INTENSITY_TARGET):
        """The quality sweep of this reference in one launch; returns one MetricResult (or error) per test."""
        config = config or MetricConfig.ssimulacra2_only()
        bufs = [_buf(t) for t in tests]
        n = len(bufs)
        if n == 0:
            return []
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (_sz * n)(*[b.size for b in bufs])
        out = (CeScores * n)()
        self.ctx._check(lib().ce_ref_compare_many(self._h, ptrs, lens, n, config.mask, intensity_target, out))
        res = []
        for s in out:
            res.append(MetricResult.from_c(s) if s.status == 0 else _error_obj(s.status, self.ctx._err()))
        return res

    def butteraugli_diffmaps(self, first: int, count: int, block: int = 1) -> np.ndarray:
        """Diffmaps of tests [first, first + count) of the last compare / compare_many (handle made with
        butteraugli_diffmap=True, a config with Butteraugli): see Batch.butteraugli_diffmaps."""
        return _read_diffmaps(self.ctx, lib().ce_ref_butteraugli_diffmap, self._h, self.width, self.height, first, count, block)

    def dssim_ssim_maps(self, level: int, first: int, count: int, block: int = 1):
        """DSSIM's SsimMap of tests [first, first + count) of the last compare / compare_many with DSSIM: see
        Batch.dssim_ssim_maps."""
        return _read_ssim_maps(self.ctx, lib().ce_ref_dssim_ssim_maps, self._h, self.width, self.height, level, first, count, block)

    def ssimulacra2_maps(self, scale: int, channel: int, kind: int, first: int, count: int, block: int = 1, maps: bool = True):
        """SSIMULACRA2's maps of tests [first, first + count) of the last compare / compare_many (maps: a handle made with
        ssimulacra2_maps=True): see Batch.ssimulacra2_maps."""
        return _read_ssim2_maps(self.ctx, lib().ce_ref_ssimulacra2_maps, self._h, self.width, self.height, scale, channel, kind,
                                first, count, block, maps)

    def image_heuristics(self, image: str = "") -> ImageHeuristics:
        """compute_heuristics of the handle's reference image."""
        out = CeImageHeuristics()
        self.ctx._check(lib().ce_ref_image_heuristics(self._h, C.byref(out)))
        return ImageHeuristics.from_c(out, image)

    def stats(self):
        """(ssimulacra2, dssim, butteraugli): compares so far that had to build that metric's reference-side state."""
        out = (_u32 * 3)()
        self.ctx._check(lib().ce_ref_stats(self._h, C.byref(out)))
        return tuple(out)

    def close(self):
        if self._h and self.ctx._h:
            lib().ce_ref_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- codec-iter's plug point (crates/codec-iter/src/eval.rs:56-92, gpu.rs:21-134) ------------
Ssimulacra2Reference = ReferenceHandle  # fast_ssim2::Ssimulacra2Reference::{new, compare}


class GpuSsim2:
    """GpuSsim2::new(w, h) / compute(&mut self, reference, distorted) (gpu.rs:40-116): fixed shape, packed
    RGB8 from host memory, one call in flight per object."""

    def __init__(self, width: int, height: int, device: int = 0):
        self.ctx = Context(device)
        self.width, self.height = int(width), int(height)

    def compute(self, reference, distorted) -> float:
        r, d = _buf(reference), _buf(distorted)
        expected = self.width * self.height * 3
        if r.size != expected or d.size != expected:  # gpu.rs:84-94
            raise RuntimeError(f"Image size mismatch: expected {expected} bytes ({self.width}x{self.height}x3), "
                               f"got ref={r.size} dis={d.size}")
        return self.ctx.calculate_ssimulacra2(r, d, self.width, self.height)

    def dimensions(self):
        return (self.width, self.height)

    def close(self):
        self.ctx.close()


class Ssim2Backend:
    """eval.rs:56-92.  The reference's enum has a Gpu and a Cpu arm; this package is the device arm and has
    no CPU path, so only that arm exists here."""

    def __init__(self, gpu: GpuSsim2):
        self.gpu = gpu

    def compare_with_precomputed(self, source, decoded, reference: Optional[ReferenceHandle], image_name: str, quality: int) -> float:
        try:
            if reference is not None:
                return reference.compare(decoded).ssimulacra2
            return self.gpu.compute(source, decoded)
        except (CodecEvalError, RuntimeError) as e:  # eval.rs:88
            raise RuntimeError(f"SSIM2 error for {image_name} q{quality}: {e}") from e


# ---- eval helpers (src/eval/helpers.rs) ----------------------------------------------------
class QualityBelowThreshold(CodecEvalError):
    def __init__(self, metric: str, value: float, threshold: float):
        RuntimeError.__init__(self, f"{metric} quality below threshold: {value} (threshold: {threshold})")
        self.status, self.kind = -1, "QualityBelowThreshold"
        self.metric, self.value, self.threshold = metric, value, threshold


def _as_rgb8(img) -> np.ndarray:
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise TypeError("expected an (h, w, 3) uint8 image")
    return a


def evaluate_single(ctx: Context, reference, encoded, config: MetricConfig) -> MetricResult:
    """evaluate_single, src/eval/helpers.rs:105-173: (h, w, 3) uint8 images."""
    r, e = _as_rgb8(reference), _as_rgb8(encoded)
    if r.shape != e.shape:  # helpers.rs:111-116
        raise DimensionMismatch(CE_ERR_DIM_MISMATCH, f"expected {(r.shape[1], r.shape[0])}, got {(e.shape[1], e.shape[0])}")
    return ctx.calculate_metrics(r, e, r.shape[1], r.shape[0], config)


def assert_quality(ctx: Context, reference, encoded, min_ssimulacra2: Optional[float], max_dssim: Optional[float]) -> None:
    """assert_quality, src/eval/helpers.rs:212-255."""
    cfg = MetricConfig(dssim=max_dssim is not None, ssimulacra2=min_ssimulacra2 is not None)
    res = evaluate_single(ctx, reference, encoded, cfg)
    if min_ssimulacra2 is not None and res.ssimulacra2 is not None and res.ssimulacra2 < min_ssimulacra2:
        raise QualityBelowThreshold("SSIMULACRA2", res.ssimulacra2, min_ssimulacra2)
    if max_dssim is not None and res.dssim is not None and res.dssim > max_dssim:
        raise QualityBelowThreshold("DSSIM", res.dssim, max_dssim)


def assert_perception_level(ctx: Context, reference, encoded, min_level: str) -> None:
    """assert_perception_level, src/eval/helpers.rs:291-321 (DSSIM only, ordinal compare)."""
    res = evaluate_single(ctx, reference, encoded, MetricConfig(dssim=True))
    if res.dssim is not None:
        actual = PERCEPTION_LEVELS.index(perception_from_dssim(res.dssim))
        want = PERCEPTION_LEVELS.index(min_level)
        if actual > want:
            raise QualityBelowThreshold(f"PerceptionLevel (DSSIM {res.dssim:.6f})", float(actual), float(want))
