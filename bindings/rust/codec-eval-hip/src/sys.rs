//! Raw declarations of `include/ce_metrics.h`.  One `pub fn` per exported symbol, same order as the header.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_float, c_int, c_void};

#[repr(C)]
pub struct ce_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ce_batch {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ce_ref {
    _private: [u8; 0],
}
#[repr(C)]
pub struct ce_lut {
    _private: [u8; 0],
}

pub const CE_OK: c_int = 0;
pub const CE_ERR_DIM_MISMATCH: c_int = 1;
pub const CE_ERR_BAD_LENGTH: c_int = 2;
pub const CE_ERR_TOO_SMALL: c_int = 3;
pub const CE_ERR_BACKEND: c_int = 4;
pub const CE_ERR_INVALID_ARG: c_int = 5;

pub const CE_METRIC_DSSIM: u32 = 1 << 0;
pub const CE_METRIC_SSIMULACRA2: u32 = 1 << 1;
pub const CE_METRIC_BUTTERAUGLI: u32 = 1 << 2;
pub const CE_METRIC_PSNR: u32 = 1 << 3;
pub const CE_FLAG_XYB_ROUNDTRIP: u32 = 1 << 0;
pub const CE_FLAG_BUTTERAUGLI_DIFFMAP: u32 = 1 << 1;
pub const CE_FLAG_SSIMULACRA2_MAPS: u32 = 1 << 2;
pub const CE_DEFAULT_INTENSITY_TARGET: c_float = 80.0;
pub const CE_DSSIM_MAX_LEVELS: usize = 5;
pub const CE_SSIM2_MAX_SCALES: usize = 6;
pub const CE_SSIM2_MAP_SSIM: u32 = 0;
pub const CE_SSIM2_MAP_ARTIFACT: u32 = 1;
pub const CE_SSIM2_MAP_DETAIL_LOST: u32 = 2;

pub const CE_PIXEL_RGB8: c_int = 0;
pub const CE_PIXEL_RGBA8: c_int = 1;
pub const CE_PIXEL_RGB16_10BIT: c_int = 2;
pub const CE_PIXEL_RGBA16_10BIT: c_int = 3;
/// deep batches only (`ce_batch_create_deep`): u16 samples at the side's own depth
pub const CE_PIXEL_RGB16: c_int = 4;
pub const CE_PIXEL_RGBA16: c_int = 5;
/// linear batches only (`ce_batch_create_linear`): packed f32 RGB, linear light with BT.709 / sRGB primaries
pub const CE_PIXEL_RGB_F32: c_int = 7;
/// packed float RGBA, 16 bytes per pixel, linear light: the `*_linear_over` calls only
pub const CE_PIXEL_RGBA_F32: c_int = 8;
/// `CE_LINEAR_MAX`: the clamp of a linear image's samples on ingest
pub const CE_LINEAR_MAX: c_float = 1024.0;

/// a matrix/TRC ICC profile on a context's device (`ce_icc_create`)
#[repr(C)]
pub struct ce_icc {
    _private: [u8; 0],
}
pub const CE_ICC_MAX_PROFILE_BYTES: usize = 4194304;
pub const CE_ICC_MAX_CURVE_POINTS: u32 = 65536;
pub const CE_ICC_SUPPORTED: c_int = 0;
pub const CE_ICC_LUT_BASED: c_int = 1;
pub const CE_ICC_NOT_RGB_XYZ: c_int = 2;
pub const CE_ICC_MALFORMED: c_int = 3;
pub const CE_ICC_CURVE_CURV: c_int = 0;
pub const CE_ICC_CURVE_PARA: c_int = 1;

/// `ce_icc_curve` (40 bytes): one tone curve of a matrix/TRC profile as the parser read it.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_icc_curve {
    pub type_: c_int,
    pub count: u32,
    pub params: [i32; 7],
    pub offset: u32,
}

/// `ce_icc_lut_describe` only: `count` u8 samples at `offset` (the tables of an `mft1` tag)
pub const CE_ICC_CURVE_TABLE8: c_int = 2;

pub const CE_ICC_MAX_CLUT_NODES: u32 = 274625;
pub const CE_ICC_LUT_SUPPORTED: c_int = 0;
pub const CE_ICC_LUT_NOT_LUT: c_int = 1;
pub const CE_ICC_LUT_UNSUPPORTED: c_int = 2;
pub const CE_ICC_LUT_MALFORMED: c_int = 3;
pub const CE_ICC_CLUT_TRILINEAR: c_int = 0;
pub const CE_ICC_CLUT_TETRAHEDRAL: c_int = 1;
pub const CE_ICC_STAGE_A: u32 = 1;
pub const CE_ICC_STAGE_CLUT: u32 = 2;
pub const CE_ICC_STAGE_M: u32 = 4;
pub const CE_ICC_STAGE_MATRIX: u32 = 8;
pub const CE_ICC_STAGE_B: u32 = 16;
pub const CE_ICC_LUT_CURVE_IDENTITY: c_int = 0;
pub const CE_ICC_LUT_CURVE_SAMPLED: c_int = 1;
pub const CE_ICC_LUT_CURVE_POWER: c_int = 2;

/// `ce_icc_lut_description` (560 bytes): what `ce_icc_lut_describe` reads from a LUT-based profile.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ce_icc_lut_description {
    pub kind: c_int,
    pub version: u32,
    pub profile_class: u32,
    pub pcs: u32,
    pub tag: u32,
    pub tag_type: u32,
    pub tag_offset: u32,
    pub tag_size: u32,
    pub stages: u32,
    pub grid: [u32; 3],
    pub precision: u32,
    pub clut_offset: u32,
    pub matrix: [i32; 12],
    pub a: [ce_icc_curve; 3],
    pub m: [ce_icc_curve; 3],
    pub b: [ce_icc_curve; 3],
    pub reason: [c_char; 96],
}

/// `ce_icc_lut_curve` (72 bytes): a post-CLUT curve as the kernel takes it.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_icc_lut_curve {
    pub kind: c_int,
    pub ftype: u32,
    pub count: u32,
    pub first_sample: u32,
    pub q: [f64; 7],
}

/// `ce_icc_description` (264 bytes): what `ce_icc_describe` reads from a profile.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ce_icc_description {
    pub kind: c_int,
    pub version: u32,
    pub profile_class: u32,
    pub colorants: [i32; 9],
    pub curves: [ce_icc_curve; 3],
    pub reason: [c_char; 96],
}

/// `ce_colour` (16 bytes): how integer RGB code values are to be read (ITU-T H.273 code points).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_colour {
    pub primaries: c_int,
    pub transfer: c_int,
    pub depth: u32,
    pub white_nits: c_float,
}

/// `ce_hlg` (20 bytes): how BT.2100 HLG code values are to be read, with the display they are shown on.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_hlg {
    pub primaries: c_int,
    pub depth: u32,
    pub peak_nits: c_float,
    /// 0: BT.2100's rule from `peak_nits`
    pub system_gamma: c_float,
    pub white_nits: c_float,
}

/// `ce_gainmap_image` (24 bytes): a gain map's samples in host memory, `height` rows of `width * channels` bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_gainmap_image {
    pub samples: *const u8,
    pub width: u32,
    pub height: u32,
    /// 1 or 3
    pub channels: u32,
}

/// `ce_gainmap` (72 bytes): a gain map's metadata; gains and headrooms are log2 values, and a single-channel map reads
/// index 0 of each array only.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct ce_gainmap {
    pub gain_min: [c_float; 3],
    pub gain_max: [c_float; 3],
    pub gamma: [c_float; 3],
    pub base_offset: [c_float; 3],
    pub alternate_offset: [c_float; 3],
    pub base_headroom: c_float,
    pub alternate_headroom: c_float,
    pub display_headroom: c_float,
}

/// `ce_hdr_scores` (48 bytes): PSNR in the PQ domain and BT.2124's Delta E ITP of one pair of a linear batch, with the three
/// exact integers they are finished from.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_hdr_scores {
    pub pq_psnr: c_double,
    pub delta_e_itp_mean: c_double,
    pub delta_e_itp_max: c_double,
    pub pq_sse: u64,
    pub itp_sum_q20: u64,
    pub itp_max_q20: u64,
}

/// `ce_msssim_scores` (352 bytes): SSIM and MS-SSIM of one pair on the encoded sample values, with the exact integers they are
/// finished from - per level and channel the sums of the per-position values in units of 2^-32 - and the positions of a level.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_msssim_scores {
    pub ms_ssim: c_double,
    pub ssim: c_double,
    pub ms_ssim_rgb: [c_double; 3],
    pub ssim_rgb: [c_double; 3],
    pub ssim_q: [[i64; 3]; 5],
    pub cs_q: [[i64; 3]; 5],
    pub n: [u64; 5],
    pub n_levels: u32,
    pub reserved: u32,
}

/// `ce_ciede2000_scores` (120 bytes): CIEDE2000 of one pair read as sRGB - the mean and the maximum of the per-pixel Delta E 2000
/// and 45 - 20 log10(mean) - with the exact integers they are finished from, in units of 2^-20, and the pixels above each threshold.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_ciede2000_scores {
    pub sum_q20: u64,
    pub n: u64,
    pub n_above: [u64; 8],
    pub mean: c_double,
    pub max: c_double,
    pub ciede2000_db: c_double,
    pub max_q20: u32,
    pub n_thresholds: u32,
    pub reserved: [u32; 2],
}

/// `ce_plane_scores` (512 bytes): one pair of Y'CbCr images scored plane by plane, index 0, 1, 2 = Y, Cb, Cr: the exact squared
/// error and sample count, the PSNRs finished from them, and per plane and level the integers of SSIM / MS-SSIM with the
/// positions of a level.  What did not run is 0 (integers) or NaN (doubles).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_plane_scores {
    pub sse: [u64; 3],
    pub n: [u64; 3],
    pub psnr: [c_double; 3],
    pub psnr_weighted: c_double,
    pub psnr_overall: c_double,
    pub ssim: [c_double; 3],
    pub ms_ssim: [c_double; 3],
    pub ssim_q: [[i64; 5]; 3],
    pub cs_q: [[i64; 5]; 3],
    pub n_pos: [[u64; 5]; 3],
    pub n_levels: [u32; 3],
    pub n_planes: u32,
}

/// `ce_plane_hvs_scores` (176 bytes): PSNR-HVS and PSNR-HVS-M of one pair of Y'CbCr images plane by plane: the exact sums as
/// [low 32 bits, the rest], the DCT blocks of a plane and the two scores.  A plane without a block has 0 and NaN.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_plane_hvs_scores {
    pub hvs_q: [[u64; 2]; 3],
    pub hvsm_q: [[u64; 2]; 3],
    pub n_blocks: [u64; 3],
    pub psnr_hvs: [c_double; 3],
    pub psnr_hvsm: [c_double; 3],
    pub n_planes: u32,
    pub step: u32,
}

/// `ce_plane_vif_scores` (424 bytes): pixel-domain VIF of one pair of Y'CbCr images plane by plane: per plane and scale the exact
/// sums of the test's and the reference's information in units of 2^-24 nat, the positions and their ratio; `vifp` over the four
/// scales.  A plane that did not run (`ran[p] == 0`) has 0 and NaN.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_plane_vif_scores {
    pub num_q: [[u64; 4]; 3],
    pub den_q: [[u64; 4]; 3],
    pub n_pos: [[u64; 4]; 3],
    pub vif_scale: [[c_double; 4]; 3],
    pub vifp: [c_double; 3],
    pub ran: [u32; 3],
    pub n_planes: u32,
}

/// `ce_plane_gmsd_scores` (160 bytes): GMSD of one pair of Y'CbCr images plane by plane: the exact sum of the gradient magnitude
/// similarities in units of 2^-32, the exact sum of their squares as [low 64 bits, high 64 bits], the positions, the deviation
/// (dividing by N), the mean and the largest 2^32 - q.  A plane the subsampling lacks has 0 and NaN.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct ce_plane_gmsd_scores {
    pub sum_q: [u64; 3],
    pub sum_q2: [[u64; 2]; 3],
    pub n_pos: [u64; 3],
    pub gmsd: [c_double; 3],
    pub gmsm: [c_double; 3],
    pub max_dis: [u32; 3],
    pub n_planes: u32,
}

/// `ce_scores` (40 bytes): a score is meaningful iff its bit is set in `valid`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ce_scores {
    pub dssim: c_double,
    pub ssimulacra2: c_double,
    pub butteraugli: c_double,
    pub psnr: c_double,
    pub valid: u32,
    pub status: i32,
}

/// `ce_image_heuristics` (128 bytes): `ImageHeuristics` of crates/codec-compare/src/image_heuristics.rs:22-63 without the
/// name, plus analyze-image's `detail_block_pct` (variance > 1000).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ce_image_heuristics {
    pub width: u64,
    pub height: u64,
    pub pixels: u64,
    pub mean_luminance: c_float,
    pub luminance_variance: c_float,
    pub luminance_std: c_float,
    pub edge_strength_mean: c_float,
    pub edge_strength_max: c_float,
    pub edge_density: c_float,
    pub flat_block_pct: c_float,
    pub low_var_block_pct: c_float,
    pub mid_var_block_pct: c_float,
    pub high_var_block_pct: c_float,
    pub detail_block_pct: c_float,
    pub block_variance_mean: c_float,
    pub block_variance_std: c_float,
    pub color_variance: c_float,
    pub saturation_mean: c_float,
    pub saturation_std: c_float,
    pub high_freq_energy: c_float,
    pub low_freq_energy: c_float,
    pub freq_ratio: c_float,
    pub local_contrast_mean: c_float,
    pub local_contrast_std: c_float,
    pub horizontal_complexity: c_float,
    pub vertical_complexity: c_float,
    pub diagonal_complexity: c_float,
    pub analyze_detail_block_pct: c_float,
}
pub const CE_BATCH_REFERENCES: u32 = 0;
pub const CE_BATCH_TESTS: u32 = 1;
/// `CE_DELTA_E_ITP_MAX_THRESHOLDS`, and a Delta E ITP of 1.0 in the units of the maps and thresholds (`CE_DELTA_E_ITP_Q20`)
pub const CE_DELTA_E_ITP_MAX_THRESHOLDS: u32 = 8;
pub const CE_DELTA_E_ITP_Q20: u32 = 1 << 20;
/// `CE_MSSSIM_MAP_MAX_THRESHOLDS`, an SSIM of 1.0 in the units of the SSIM / MS-SSIM maps and thresholds (`CE_MSSSIM_Q32`), and
/// the two terms a map can hold (`CE_MSSSIM_MAP_SSIM`, `CE_MSSSIM_MAP_CS`)
pub const CE_MSSSIM_MAP_MAX_THRESHOLDS: u32 = 8;
pub const CE_MSSSIM_Q32: u64 = 1 << 32;
pub const CE_MSSSIM_MAP_SSIM: u32 = 0;
pub const CE_MSSSIM_MAP_CS: u32 = 1;
/// `CE_CIEDE2000_MAX_THRESHOLDS`, a CIEDE2000 of 1.0 in the units of q, the maps and the thresholds (`CE_CIEDE2000_Q20`), and the
/// four values a CIEDE2000 map can hold: q itself or the magnitude of its lightness, chroma or hue term (`CE_CIEDE2000_MAP_*`)
pub const CE_CIEDE2000_MAX_THRESHOLDS: u32 = 8;
pub const CE_CIEDE2000_Q20: u32 = 1 << 20;
pub const CE_CIEDE2000_MAP_DE: u32 = 0;
pub const CE_CIEDE2000_MAP_DL: u32 = 1;
pub const CE_CIEDE2000_MAP_DC: u32 = 2;
pub const CE_CIEDE2000_MAP_DH: u32 = 3;

/// `ce_pair_desc` (40 bytes): one item of the (image x codec x quality) grid, host pointers.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_pair_desc {
    pub reference: *const u8,
    pub reference_len: usize,
    pub test: *const u8,
    pub test_len: usize,
    pub width: u32,
    pub height: u32,
}

// planar Y'CbCr ingest
pub const CE_YUV_444: c_int = 0;
pub const CE_YUV_422: c_int = 1;
pub const CE_YUV_420: c_int = 2;
pub const CE_YUV_400: c_int = 3;
pub const CE_YUV_PLANAR: c_int = 0;
pub const CE_YUV_SEMIPLANAR: c_int = 1;
pub const CE_YUV_BT601: c_int = 0;
pub const CE_YUV_BT709: c_int = 1;
pub const CE_YUV_BT2020: c_int = 2;
pub const CE_YUV_FULL: c_int = 0;
pub const CE_YUV_LIMITED: c_int = 1;
pub const CE_CHROMA_NEAREST: c_int = 0;
pub const CE_CHROMA_TRIANGLE: c_int = 1;
pub const CE_MEM_HOST: c_int = 0;
pub const CE_MEM_DEVICE: c_int = 1;

// enum ce_dtype, enum ce_quantise: the tensor ingest
pub const CE_DTYPE_U8: c_int = 0;
pub const CE_DTYPE_U16: c_int = 1;
pub const CE_DTYPE_F16: c_int = 2;
pub const CE_DTYPE_BF16: c_int = 3;
pub const CE_DTYPE_F32: c_int = 4;
pub const CE_QUANT_NEAREST_EVEN: c_int = 0;
pub const CE_QUANT_TRUNCATE: c_int = 1;

/// `ce_tensor_image` (56 bytes): a framework's strided image tensor, in host or device memory; strides in ELEMENTS.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_tensor_image {
    pub data: *const c_void,
    pub stride_n: i64,
    pub stride_c: i64,
    pub stride_y: i64,
    pub stride_x: i64,
    pub dtype: c_int,
    pub memory: c_int,
    pub quantise: c_int,
}

/// `CE_MAX_BACKGROUNDS`: solid colours one upload is composited over
pub const CE_MAX_BACKGROUNDS: usize = 8;

/// `ce_yuv_image` (88 bytes): a decoder's Y'CbCr planes, in host or device memory.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ce_yuv_image {
    pub plane: [*const c_void; 3],
    pub pitch: [usize; 3],
    pub subsampling: c_int,
    pub layout: c_int,
    pub matrix: c_int,
    pub range: c_int,
    pub upsample: c_int,
    pub depth: c_int,
    pub msb_aligned: c_int,
    pub memory: c_int,
    pub lut: *const ce_lut,
}

extern "C" {
    pub fn ce_version() -> *const c_char;
    pub fn ce_device_count() -> c_int;
    pub fn ce_ctx_create(device: c_int, out: *mut *mut ce_ctx) -> c_int;
    pub fn ce_ctx_create_on_stream(device: c_int, hip_stream: *mut c_void, out: *mut *mut ce_ctx) -> c_int;
    pub fn ce_ctx_destroy(ctx: *mut ce_ctx);
    pub fn ce_ctx_synchronize(ctx: *mut ce_ctx) -> c_int;
    pub fn ce_ctx_stream(ctx: *mut ce_ctx) -> *mut c_void;
    pub fn ce_last_error(ctx: *const ce_ctx) -> *const c_char;
    pub fn ce_calculate_psnr(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                             width: usize, height: usize, out: *mut c_double) -> c_int;
    pub fn ce_calculate_ssimulacra2(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                    width: usize, height: usize, out: *mut c_double) -> c_int;
    pub fn ce_calculate_dssim(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                              width: usize, height: usize, out: *mut c_double) -> c_int;
    pub fn ce_calculate_butteraugli(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                    width: usize, height: usize, intensity_target: c_float, out: *mut c_double) -> c_int;
    pub fn ce_calculate_butteraugli_diffmap(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8,
                                            test_len: usize, width: usize, height: usize, intensity_target: c_float,
                                            score: *mut c_double, diffmap_out: *mut c_float) -> c_int;
    pub fn ce_dssim_levels(width: u32, height: u32, n_levels: *mut u32, level_w: *mut u32, level_h: *mut u32) -> c_int;
    pub fn ce_calculate_dssim_ssim_maps(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                        width: usize, height: usize, dssim: *mut c_double, level_ssim: *mut c_double,
                                        maps: *mut c_float, maps_floats: usize) -> c_int;
    pub fn ce_ssimulacra2_scales(width: u32, height: u32, n_scales: *mut u32, scale_w: *mut u32, scale_h: *mut u32) -> c_int;
    pub fn ce_calculate_ssimulacra2_maps(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                         width: usize, height: usize, score: *mut c_double, features: *mut c_double,
                                         maps: *mut c_float, maps_floats: usize) -> c_int;
    pub fn ce_xyb_roundtrip(ctx: *mut ce_ctx, rgb: *const u8, rgb_len: usize, width: usize, height: usize, out: *mut u8) -> c_int;
    pub fn ce_rgb8_to_dssim_image(ctx: *mut ce_ctx, rgb: *const u8, rgb_len: usize, width: usize, height: usize,
                                  out_rgba_f32: *mut c_float) -> c_int;
    pub fn ce_eval_pair(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                        width: u32, height: u32, metric_mask: u32, flags: u32, intensity_target: c_float,
                        out: *mut ce_scores) -> c_int;
    pub fn ce_eval_batch(ctx: *mut ce_ctx, n: usize, pairs: *const ce_pair_desc, metric_mask: u32, flags: u32,
                         intensity_target: c_float, out: *mut ce_scores) -> c_int;
    pub fn ce_estimate_batch_bytes(width: u32, height: u32, n_refs: u32, n_pairs: u32, metric_mask: u32) -> usize;
    pub fn ce_ctx_memory_info(ctx: *mut ce_ctx, free_bytes: *mut usize, total_bytes: *mut usize) -> c_int;
    pub fn ce_host_alloc(ctx: *mut ce_ctx, bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn ce_host_free(ctx: *mut ce_ctx, p: *mut c_void) -> c_int;
    pub fn ce_eval_batch_lut(ctx: *mut ce_ctx, n: usize, pairs: *const ce_pair_desc, test_luts: *const *const ce_lut, metric_mask: u32,
                             flags: u32, intensity_target: c_float, out: *mut ce_scores) -> c_int;
    pub fn ce_batch_create(ctx: *mut ce_ctx, width: u32, height: u32, max_refs: u32, max_pairs: u32, out: *mut *mut ce_batch) -> c_int;
    pub fn ce_batch_destroy(b: *mut ce_batch);
    pub fn ce_pixel_bytes(format: c_int) -> usize;
    pub fn ce_batch_create_deep(ctx: *mut ce_ctx, width: u32, height: u32, max_refs: u32, max_pairs: u32, ref_depth: u32,
                                test_depth: u32, out: *mut *mut ce_batch) -> c_int;
    pub fn ce_estimate_batch_bytes_deep(width: u32, height: u32, n_refs: u32, n_pairs: u32, metric_mask: u32, ref_depth: u32,
                                        test_depth: u32) -> usize;
    pub fn ce_eval_pair_deep(ctx: *mut ce_ctx, reference: *const u16, reference_len: usize, ref_depth: u32, test: *const u16,
                             test_len: usize, test_depth: u32, width: u32, height: u32, metric_mask: u32, flags: u32,
                             intensity_target: c_float, out: *mut ce_scores) -> c_int;
    pub fn ce_batch_create_linear(ctx: *mut ce_ctx, width: u32, height: u32, max_refs: u32, max_pairs: u32, out: *mut *mut ce_batch) -> c_int;
    pub fn ce_estimate_batch_bytes_linear(width: u32, height: u32, n_refs: u32, n_pairs: u32, metric_mask: u32) -> usize;
    pub fn ce_eval_pair_linear(ctx: *mut ce_ctx, reference: *const c_float, reference_len: usize, test: *const c_float, test_len: usize,
                               width: u32, height: u32, metric_mask: u32, flags: u32, intensity_target: c_float,
                               out: *mut ce_scores) -> c_int;
    pub fn ce_srgb_table(depth: u32, rule: c_int, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_batch_set_reference_cicp(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                       c: *const ce_colour) -> c_int;
    pub fn ce_batch_set_test_cicp(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                  c: *const ce_colour) -> c_int;
    pub fn ce_cicp_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, c: *const ce_colour, w: u32, h: u32,
                             out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_transfer_table(transfer: c_int, depth: u32, white_nits: c_float, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_colour_matrix(primaries: c_int, out: *mut c_float) -> c_int;
    pub fn ce_batch_set_reference(b: *mut ce_batch, ref_index: u32, rgb: *const u8, len: usize) -> c_int;
    pub fn ce_batch_set_test(b: *mut ce_batch, pair_index: u32, ref_index: u32, rgb: *const u8, len: usize) -> c_int;
    pub fn ce_batch_set_reference_fmt(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int) -> c_int;
    pub fn ce_batch_set_test_fmt(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize,
                                 format: c_int) -> c_int;
    pub fn ce_lut_create(ctx: *mut ce_ctx, table: *const u8, table_len: usize, out: *mut *mut ce_lut) -> c_int;
    pub fn ce_lut_destroy(lut: *mut ce_lut);
    pub fn ce_batch_set_reference_lut(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                      lut: *const ce_lut) -> c_int;
    pub fn ce_batch_set_test_lut(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                 lut: *const ce_lut) -> c_int;
    pub fn ce_batch_reference_slab(b: *mut ce_batch) -> *mut c_void;
    pub fn ce_batch_references_changed(b: *mut ce_batch) -> c_int;
    pub fn ce_batch_ref_stats(b: *const ce_batch, builds: *mut u32) -> c_int;
    pub fn ce_batch_test_slab(b: *mut ce_batch) -> *mut c_void;
    pub fn ce_batch_bind_pair(b: *mut ce_batch, pair_index: u32, ref_index: u32) -> c_int;
    pub fn ce_batch_run(b: *mut ce_batch, n_pairs: u32, metric_mask: u32, flags: u32, intensity_target: c_float,
                        out: *mut ce_scores) -> c_int;
    pub fn ce_batch_launch(b: *mut ce_batch, n_pairs: u32, metric_mask: u32, flags: u32, intensity_target: c_float) -> c_int;
    pub fn ce_batch_collect(b: *mut ce_batch, n_pairs: u32, out: *mut ce_scores) -> c_int;
    pub fn ce_batch_butteraugli_pnorm3(b: *mut ce_batch, n_pairs: u32, out: *mut c_double) -> c_int;
    pub fn ce_batch_butteraugli_diffmap(b: *mut ce_batch, first: u32, count: u32, block: u32, out: *mut c_float,
                                        out_floats: usize) -> c_int;
    pub fn ce_batch_dssim_ssim_maps(b: *mut ce_batch, level: u32, first: u32, count: u32, block: u32, maps: *mut c_float,
                                    maps_floats: usize, ssim: *mut c_double) -> c_int;
    pub fn ce_batch_ssimulacra2_maps(b: *mut ce_batch, scale: u32, channel: u32, kind: u32, first: u32, count: u32, block: u32,
                                     maps: *mut c_float, maps_floats: usize, norms: *mut c_double) -> c_int;
    pub fn ce_ref_create(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, width: u32, height: u32, flags: u32,
                         out: *mut *mut ce_ref) -> c_int;
    pub fn ce_ref_compare(r: *mut ce_ref, test: *const u8, test_len: usize, metric_mask: u32, intensity_target: c_float,
                          out: *mut ce_scores) -> c_int;
    pub fn ce_ref_compare_many(r: *mut ce_ref, tests: *const *const u8, test_lens: *const usize, n_tests: u32, metric_mask: u32,
                               intensity_target: c_float, out: *mut ce_scores) -> c_int;
    pub fn ce_ref_stats(r: *const ce_ref, builds: *mut u32) -> c_int;
    pub fn ce_ref_butteraugli_diffmap(r: *mut ce_ref, first: u32, count: u32, block: u32, out: *mut c_float,
                                      out_floats: usize) -> c_int;
    pub fn ce_ref_dssim_ssim_maps(r: *mut ce_ref, level: u32, first: u32, count: u32, block: u32, maps: *mut c_float,
                                  maps_floats: usize, ssim: *mut c_double) -> c_int;
    pub fn ce_ref_ssimulacra2_maps(r: *mut ce_ref, scale: u32, channel: u32, kind: u32, first: u32, count: u32, block: u32,
                                   maps: *mut c_float, maps_floats: usize, norms: *mut c_double) -> c_int;
    pub fn ce_ref_destroy(r: *mut ce_ref);
    pub fn ce_image_heuristics_rgb8(ctx: *mut ce_ctx, rgb: *const u8, len: usize, width: usize, height: usize,
                                    out: *mut ce_image_heuristics) -> c_int;
    pub fn ce_batch_image_heuristics(b: *mut ce_batch, which: u32, first: u32, count: u32, out: *mut ce_image_heuristics) -> c_int;
    pub fn ce_ref_image_heuristics(r: *mut ce_ref, out: *mut ce_image_heuristics) -> c_int;
    pub fn ce_resample_rgb8(ctx: *mut ce_ctx, rgb: *const u8, len: usize, w: u32, h: u32, out_w: u32, out_h: u32, filter: c_int,
                            out: *mut u8, out_len: usize) -> c_int;
    pub fn ce_resample_linear(ctx: *mut ce_ctx, rgb: *const c_float, len: usize, w: u32, h: u32, out_w: u32, out_h: u32, filter: c_int,
                              out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_batch_resample(src: *mut ce_batch, dst: *mut ce_batch, which: u32, first: u32, count: u32, filter: c_int) -> c_int;
    pub fn ce_batch_resample_pairs(src: *mut ce_batch, dst: *mut ce_batch, n_refs: u32, n_pairs: u32, filter: c_int) -> c_int;
    pub fn ce_yuv_coefficients(matrix: c_int, range: c_int, depth_in: u32, depth_out: u32, out: *mut i64) -> c_int;
    pub fn ce_batch_set_reference_yuv(b: *mut ce_batch, ref_index: u32, image: *const ce_yuv_image) -> c_int;
    pub fn ce_batch_set_test_yuv(b: *mut ce_batch, pair_index: u32, ref_index: u32, image: *const ce_yuv_image) -> c_int;
    pub fn ce_yuv_to_rgb8(ctx: *mut ce_ctx, image: *const ce_yuv_image, width: u32, height: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn ce_yuv_to_rgb16(ctx: *mut ce_ctx, image: *const ce_yuv_image, width: u32, height: u32, depth_out: u32, out: *mut u16,
                           out_len: usize) -> c_int;
    pub fn ce_batch_set_reference_yuv_cicp(b: *mut ce_batch, ref_index: u32, image: *const ce_yuv_image, c: *const ce_colour) -> c_int;
    pub fn ce_batch_set_test_yuv_cicp(b: *mut ce_batch, pair_index: u32, ref_index: u32, image: *const ce_yuv_image,
                                      c: *const ce_colour) -> c_int;
    pub fn ce_yuv_to_linear(ctx: *mut ce_ctx, image: *const ce_yuv_image, c: *const ce_colour, width: u32, height: u32, out: *mut c_float,
                            out_len: usize) -> c_int;
    pub fn ce_batch_set_reference_yuv_icc(b: *mut ce_batch, ref_index: u32, image: *const ce_yuv_image, rgb_depth: u32, icc: *const ce_icc) -> c_int;
    pub fn ce_batch_set_test_yuv_icc(b: *mut ce_batch, pair_index: u32, ref_index: u32, image: *const ce_yuv_image, rgb_depth: u32,
                                     icc: *const ce_icc) -> c_int;
    pub fn ce_yuv_icc_to_linear(ctx: *mut ce_ctx, image: *const ce_yuv_image, rgb_depth: u32, icc: *const ce_icc, width: u32, height: u32,
                                out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_yuv_icc_to_srgb8(ctx: *mut ce_ctx, image: *const ce_yuv_image, rgb_depth: u32, icc: *const ce_icc, width: u32, height: u32,
                               out: *mut u8, out_len: usize) -> c_int;
    pub fn ce_yuv_icc_to_srgb16(ctx: *mut ce_ctx, image: *const ce_yuv_image, rgb_depth: u32, icc: *const ce_icc, width: u32, height: u32,
                                depth_out: u32, out: *mut u16, out_len: usize) -> c_int;
    pub fn ce_batch_set_reference_hlg(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                      h: *const ce_hlg) -> c_int;
    pub fn ce_batch_set_test_hlg(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                 h: *const ce_hlg) -> c_int;
    pub fn ce_hlg_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, h: *const ce_hlg, w: u32, height: u32,
                            out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_batch_set_reference_yuv_hlg(b: *mut ce_batch, ref_index: u32, image: *const ce_yuv_image, h: *const ce_hlg) -> c_int;
    pub fn ce_batch_set_test_yuv_hlg(b: *mut ce_batch, pair_index: u32, ref_index: u32, image: *const ce_yuv_image,
                                     h: *const ce_hlg) -> c_int;
    pub fn ce_yuv_hlg_to_linear(ctx: *mut ce_ctx, image: *const ce_yuv_image, h: *const ce_hlg, width: u32, height: u32, out: *mut c_float,
                                out_len: usize) -> c_int;
    pub fn ce_batch_set_reference_tensor(b: *mut ce_batch, first_ref: u32, count: u32, t: *const ce_tensor_image) -> c_int;
    pub fn ce_batch_set_test_tensor(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, count: u32, t: *const ce_tensor_image) -> c_int;
    pub fn ce_tensor_to_rgb8(ctx: *mut ce_ctx, t: *const ce_tensor_image, w: u32, h: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn ce_tensor_to_rgb16(ctx: *mut ce_ctx, t: *const ce_tensor_image, w: u32, h: u32, depth_out: u32, out: *mut u16, out_len: usize) -> c_int;
    pub fn ce_tensor_to_linear(ctx: *mut ce_ctx, t: *const ce_tensor_image, w: u32, h: u32, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_hlg_table(depth: u32, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_hlg_params(h: *const ce_hlg, out: *mut c_double) -> c_int;
    pub fn ce_batch_set_reference_gainmap(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                          c: *const ce_colour, map: *const ce_gainmap_image, g: *const ce_gainmap) -> c_int;
    pub fn ce_batch_set_test_gainmap(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                     c: *const ce_colour, map: *const ce_gainmap_image, g: *const ce_gainmap) -> c_int;
    pub fn ce_gainmap_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, c: *const ce_colour,
                                map: *const ce_gainmap_image, g: *const ce_gainmap, w: u32, h: u32, out: *mut c_float,
                                out_len: usize) -> c_int;
    pub fn ce_gainmap_tables(g: *const ce_gainmap, channels: u32, out: *mut c_double, n: usize) -> c_int;
    pub fn ce_gainmap_weight(g: *const ce_gainmap, w: *mut c_double) -> c_int;
    pub fn ce_batch_hdr_fidelity(b: *mut ce_batch, n_pairs: u32, depth: u32, white_nits: c_float, out: *mut ce_hdr_scores) -> c_int;
    pub fn ce_eval_pair_hdr_fidelity(ctx: *mut ce_ctx, reference: *const c_float, reference_len: usize, test: *const c_float,
                                     test_len: usize, width: u32, height: u32, depth: u32, white_nits: c_float,
                                     out: *mut ce_hdr_scores) -> c_int;
    pub fn ce_pq_code_thresholds(depth: u32, white_nits: c_float, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_hdr_fidelity_matrices(a: *mut c_float, b: *mut c_float) -> c_int;
    pub fn ce_batch_msssim(b: *mut ce_batch, n_pairs: u32, levels: u32, out: *mut ce_msssim_scores) -> c_int;
    pub fn ce_eval_pair_msssim(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize, width: u32,
                               height: u32, levels: u32, out: *mut ce_msssim_scores) -> c_int;
    pub fn ce_eval_pair_msssim_deep(ctx: *mut ce_ctx, reference: *const u16, reference_len: usize, test: *const u16, test_len: usize,
                                    depth: u32, width: u32, height: u32, levels: u32, out: *mut ce_msssim_scores) -> c_int;
    pub fn ce_batch_msssim_map(b: *mut ce_batch, first: u32, count: u32, levels: u32, level: u32, what: u32, block: u32, map: *mut u32,
                               map_len: usize, thresholds_q32: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_eval_pair_msssim_map(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                   width: u32, height: u32, levels: u32, level: u32, what: u32, block: u32, map: *mut u32, map_len: usize,
                                   thresholds_q32: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_eval_pair_msssim_map_deep(ctx: *mut ce_ctx, reference: *const u16, reference_len: usize, test: *const u16, test_len: usize,
                                        depth: u32, width: u32, height: u32, levels: u32, level: u32, what: u32, block: u32,
                                        map: *mut u32, map_len: usize, thresholds_q32: *const u32, n_thresholds: u32,
                                        over: *mut u64) -> c_int;
    pub fn ce_msssim_window(out: *mut c_double) -> c_int;
    pub fn ce_batch_ciede2000(b: *mut ce_batch, n_pairs: u32, thresholds_q20: *const u32, n_thresholds: u32, out: *mut ce_ciede2000_scores) -> c_int;
    pub fn ce_eval_pair_ciede2000(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize, width: u32,
                                  height: u32, thresholds_q20: *const u32, n_thresholds: u32, out: *mut ce_ciede2000_scores) -> c_int;
    pub fn ce_eval_pair_ciede2000_deep(ctx: *mut ce_ctx, reference: *const u16, reference_len: usize, test: *const u16, test_len: usize,
                                       ref_depth: u32, test_depth: u32, width: u32, height: u32, thresholds_q20: *const u32,
                                       n_thresholds: u32, out: *mut ce_ciede2000_scores) -> c_int;
    pub fn ce_ciede2000_pixels(ref_rgb: *const u16, ref_depth: u32, test_rgb: *const u16, test_depth: u32, n: usize, out_q20: *mut u32) -> c_int;
    pub fn ce_batch_ciede2000_map(b: *mut ce_batch, first: u32, count: u32, what: u32, block: u32, map: *mut u32, map_len: usize,
                                  thresholds_q20: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_eval_pair_ciede2000_map(ctx: *mut ce_ctx, reference: *const u8, reference_len: usize, test: *const u8, test_len: usize,
                                      width: u32, height: u32, what: u32, block: u32, map: *mut u32, map_len: usize,
                                      thresholds_q20: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_eval_pair_ciede2000_map_deep(ctx: *mut ce_ctx, reference: *const u16, reference_len: usize, test: *const u16, test_len: usize,
                                           ref_depth: u32, test_depth: u32, width: u32, height: u32, what: u32, block: u32, map: *mut u32,
                                           map_len: usize, thresholds_q20: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_ciede2000_pixel_terms(ref_rgb: *const u16, ref_depth: u32, test_rgb: *const u16, test_depth: u32, n: usize, out: *mut u32) -> c_int;
    pub fn ce_msssim_levels(w: u32, h: u32, levels: u32, n_levels: *mut u32, level_w: *mut u32, level_h: *mut u32) -> c_int;
    pub fn ce_yuv_plane_fidelity(ctx: *mut ce_ctx, width: u32, height: u32, refs: *const ce_yuv_image, n_refs: u32, tests: *const ce_yuv_image,
                                 n_pairs: u32, pair_ref: *const u32, levels: u32, out: *mut ce_plane_scores) -> c_int;
    pub fn ce_yuv_plane_hvs(ctx: *mut ce_ctx, width: u32, height: u32, refs: *const ce_yuv_image, n_refs: u32, tests: *const ce_yuv_image,
                            n_pairs: u32, pair_ref: *const u32, step: u32, out: *mut ce_plane_hvs_scores) -> c_int;
    pub fn ce_yuv_plane_vif(ctx: *mut ce_ctx, width: u32, height: u32, refs: *const ce_yuv_image, n_refs: u32, tests: *const ce_yuv_image,
                            n_pairs: u32, pair_ref: *const u32, out: *mut ce_plane_vif_scores) -> c_int;
    pub fn ce_vif_window(scale: u32, out: *mut c_double) -> c_int;
    pub fn ce_yuv_plane_gmsd(ctx: *mut ce_ctx, width: u32, height: u32, refs: *const ce_yuv_image, n_refs: u32, tests: *const ce_yuv_image,
                             n_pairs: u32, pair_ref: *const u32, out: *mut ce_plane_gmsd_scores) -> c_int;
    pub fn ce_batch_delta_e_itp_map(b: *mut ce_batch, first: u32, count: u32, depth: u32, white_nits: c_float, block: u32, map: *mut u32,
                                    map_len: usize, thresholds_q20: *const u32, n_thresholds: u32, over: *mut u64) -> c_int;
    pub fn ce_eval_pair_delta_e_itp_map(ctx: *mut ce_ctx, reference: *const c_float, reference_len: usize, test: *const c_float,
                                        test_len: usize, width: u32, height: u32, depth: u32, white_nits: c_float, block: u32,
                                        map: *mut u32, map_len: usize, thresholds_q20: *const u32, n_thresholds: u32,
                                        over: *mut u64) -> c_int;
    pub fn ce_batch_set_reference_over(b: *mut ce_batch, first_ref: u32, pixels: *const c_void, len: usize, format: c_int, n_bg: u32,
                                       backgrounds: *const u16) -> c_int;
    pub fn ce_batch_set_test_over(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, pixels: *const c_void, len: usize,
                                  format: c_int, n_bg: u32, backgrounds: *const u16) -> c_int;
    pub fn ce_composite_rgba8(ctx: *mut ce_ctx, rgba: *const u8, len: usize, w: u32, h: u32, bg: *const u8, out: *mut u8,
                              out_len: usize) -> c_int;
    pub fn ce_composite_rgba16(ctx: *mut ce_ctx, rgba: *const u16, len: usize, w: u32, h: u32, depth: u32, bg: *const u16,
                               out: *mut u16, out_len: usize) -> c_int;
    pub fn ce_icc_describe(bytes: *const u8, len: usize, out: *mut ce_icc_description) -> c_int;
    pub fn ce_icc_build_matrix(bytes: *const u8, len: usize, out: *mut c_float) -> c_int;
    pub fn ce_icc_build_tables(bytes: *const u8, len: usize, depth: u32, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_srgb_encode_thresholds(depth: u32, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_icc_create(ctx: *mut ce_ctx, bytes: *const u8, len: usize, out: *mut *mut ce_icc) -> c_int;
    pub fn ce_icc_destroy(icc: *mut ce_icc);
    pub fn ce_icc_lut_describe(bytes: *const u8, len: usize, intent: c_int, out: *mut ce_icc_lut_description) -> c_int;
    pub fn ce_icc_lut_build_input_tables(bytes: *const u8, len: usize, intent: c_int, depth: u32, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_icc_lut_build_clut(bytes: *const u8, len: usize, intent: c_int, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_icc_lut_build_matrix(bytes: *const u8, len: usize, intent: c_int, out: *mut c_float) -> c_int;
    pub fn ce_icc_lut_build_curves(bytes: *const u8, len: usize, intent: c_int, out: *mut ce_icc_lut_curve, samples: *mut c_float,
                                   n_samples: usize, needed: *mut usize) -> c_int;
    pub fn ce_icc_lut_build_pcs_matrix(out: *mut c_float) -> c_int;
    pub fn ce_icc_lut_create(ctx: *mut ce_ctx, bytes: *const u8, len: usize, intent: c_int, interpolation: c_int,
                             out: *mut *mut ce_icc) -> c_int;
    pub fn ce_batch_set_reference_icc(b: *mut ce_batch, ref_index: u32, pixels: *const c_void, len: usize, format: c_int, depth: u32,
                                      icc: *const ce_icc) -> c_int;
    pub fn ce_batch_set_test_icc(b: *mut ce_batch, pair_index: u32, ref_index: u32, pixels: *const c_void, len: usize, format: c_int,
                                 depth: u32, icc: *const ce_icc) -> c_int;
    pub fn ce_icc_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, depth: u32, icc: *const ce_icc, w: u32,
                            h: u32, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_icc_to_srgb8(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, depth: u32, icc: *const ce_icc, w: u32,
                           h: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn ce_icc_to_srgb16(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, depth: u32, icc: *const ce_icc, w: u32,
                            h: u32, depth_out: u32, out: *mut u16, out_len: usize) -> c_int;
    pub fn ce_alpha_table(depth: u32, out: *mut c_float, n: usize) -> c_int;
    pub fn ce_batch_set_reference_cicp_over(b: *mut ce_batch, first_ref: u32, pixels: *const c_void, len: usize, format: c_int,
                                            c: *const ce_colour, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_test_cicp_over(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, pixels: *const c_void, len: usize,
                                       format: c_int, c: *const ce_colour, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_reference_hlg_over(b: *mut ce_batch, first_ref: u32, pixels: *const c_void, len: usize, format: c_int,
                                           h: *const ce_hlg, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_test_hlg_over(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, pixels: *const c_void, len: usize,
                                      format: c_int, h: *const ce_hlg, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_reference_icc_over(b: *mut ce_batch, first_ref: u32, pixels: *const c_void, len: usize, format: c_int, depth: u32,
                                           icc: *const ce_icc, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_test_icc_over(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, pixels: *const c_void, len: usize,
                                      format: c_int, depth: u32, icc: *const ce_icc, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_reference_linear_over(b: *mut ce_batch, first_ref: u32, pixels: *const c_void, len: usize, format: c_int,
                                              premultiplied: c_int, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_batch_set_test_linear_over(b: *mut ce_batch, first_pair: u32, ref_indices: *const u32, pixels: *const c_void, len: usize,
                                         format: c_int, premultiplied: c_int, n_bg: u32, backgrounds: *const c_float) -> c_int;
    pub fn ce_cicp_over_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, c: *const ce_colour, w: u32, h: u32,
                                  bg: *const c_float, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_hlg_over_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, hd: *const ce_hlg, w: u32, h: u32,
                                 bg: *const c_float, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_icc_over_to_linear(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, depth: u32, icc: *const ce_icc,
                                 w: u32, h: u32, bg: *const c_float, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_linear_over(ctx: *mut ce_ctx, pixels: *const c_void, len: usize, format: c_int, premultiplied: c_int, w: u32, h: u32,
                          bg: *const c_float, out: *mut c_float, out_len: usize) -> c_int;
    pub fn ce_prof_enable(ctx: *mut ce_ctx, on: c_int) -> c_int;
    pub fn ce_prof_filter(ctx: *mut ce_ctx, substring: *const c_char) -> c_int;
    pub fn ce_prof_reset(ctx: *mut ce_ctx) -> c_int;
    pub fn ce_prof_count(ctx: *mut ce_ctx) -> c_int;
    pub fn ce_prof_get(ctx: *mut ce_ctx, index: c_int, name: *mut *const c_char, launches: *mut u64, total_ms: *mut c_double) -> c_int;
    pub fn ce_timer_start(ctx: *mut ce_ctx) -> c_int;
    pub fn ce_timer_stop(ctx: *mut ce_ctx, elapsed_ms: *mut c_double) -> c_int;
    pub fn ce_debug_ssim2_planes(b: *mut ce_batch, scale: c_int, which: c_int, channel: c_int, out: *mut c_float, out_floats: usize,
                                 w_out: *mut u32, h_out: *mut u32) -> c_int;
    pub fn ce_debug_ssim2_limit_scales(b: *mut ce_batch, max_scales: c_int) -> c_int;
    pub fn ce_debug_ssim2_averages(b: *mut ce_batch, pair_index: u32, avg: *mut c_double, n_scales: *mut c_int) -> c_int;
    pub fn ce_debug_ssim2_occupancy(which: c_int) -> c_int;
    pub fn ce_debug_cbrt_sweep(ctx: *mut ce_ctx, first_bits: u32, count: u64, mismatches: *mut u64, slow_path: *mut u64) -> c_int;
    pub fn ce_debug_div_sweep(ctx: *mut ce_ctx, seed: u64, count: u64, mismatches: *mut u64) -> c_int;
    pub fn ce_debug_calibrate_traffic(ctx: *mut ce_ctx, bytes: usize) -> c_int;
    pub fn ce_debug_dssim_walk_rows(b: *mut ce_batch, rows: u32) -> c_int;
}
