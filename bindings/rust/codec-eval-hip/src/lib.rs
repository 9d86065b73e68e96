//! Safe wrappers over `libce_metrics_hip.so` shaped like the call sites they replace in codec-eval:
//!
//! * [`HipMetrics::calculate_metrics`]  — `EvalSession::calculate_metrics` (src/eval/session.rs:437-497)
//! * [`HipMetrics::evaluate_grid`]      — the `codec x quality` sweep of `evaluate_image` as ONE device batch
//! * [`HipSsim2Reference`]              — `Ssimulacra2Reference::{new, compare}` (crates/codec-iter/src/eval.rs:138-149)
//!   plus `compare_many`, the whole quality loop of `run_eval` in one launch
//! * [`HipSsim2`]                       — `GpuSsim2::{new, compute}` (crates/codec-iter/src/gpu.rs:40-116)
//!
//! One call in flight per context (`&mut self`, like `GpuSsim2::compute`); any number of contexts per device.
pub mod sys;

use std::ffi::CStr;
use std::ptr;

/// The two error kinds the metric path produces in codec-eval (`Error::DimensionMismatch`,
/// `Error::MetricCalculation`, src/error.rs) — convert with `From` at the call site.
#[derive(Debug, thiserror::Error)]
pub enum HipError {
    #[error("Dimension mismatch: expected {expected:?}, got {actual:?}")]
    DimensionMismatch { expected: (usize, usize), actual: (usize, usize) },
    #[error("Metric calculation failed: {metric}: {reason}")]
    MetricCalculation { metric: String, reason: String },
}

/// `MetricConfig` (src/metrics/mod.rs:46-63) as the ABI's mask + flags.
#[derive(Clone, Copy, Debug, Default)]
pub struct Metrics {
    pub dssim: bool,
    pub ssimulacra2: bool,
    pub butteraugli: bool,
    pub psnr: bool,
    pub xyb_roundtrip: bool,
}

impl Metrics {
    fn mask(&self) -> u32 {
        (self.dssim as u32) * sys::CE_METRIC_DSSIM
            | (self.ssimulacra2 as u32) * sys::CE_METRIC_SSIMULACRA2
            | (self.butteraugli as u32) * sys::CE_METRIC_BUTTERAUGLI
            | (self.psnr as u32) * sys::CE_METRIC_PSNR
    }
    fn flags(&self) -> u32 {
        if self.xyb_roundtrip { sys::CE_FLAG_XYB_ROUNDTRIP } else { 0 }
    }
}

/// `MetricResult` (src/metrics/mod.rs:140-149).
#[derive(Clone, Copy, Debug, Default)]
pub struct Scores {
    pub dssim: Option<f64>,
    pub ssimulacra2: Option<f64>,
    pub butteraugli: Option<f64>,
    pub psnr: Option<f64>,
}

impl From<sys::ce_scores> for Scores {
    fn from(s: sys::ce_scores) -> Self {
        let pick = |bit: u32, v: f64| if s.valid & bit != 0 { Some(v) } else { None };
        Scores {
            dssim: pick(sys::CE_METRIC_DSSIM, s.dssim),
            ssimulacra2: pick(sys::CE_METRIC_SSIMULACRA2, s.ssimulacra2),
            butteraugli: pick(sys::CE_METRIC_BUTTERAUGLI, s.butteraugli),
            psnr: pick(sys::CE_METRIC_PSNR, s.psnr),
        }
    }
}

/// A device context (`GpuSsim2::new` / `Drop`, gpu.rs:40-80,118-133).
pub struct HipMetrics {
    ctx: *mut sys::ce_ctx,
}

unsafe impl Send for HipMetrics {}

impl HipMetrics {
    pub fn new(device: i32) -> Result<Self, HipError> {
        // HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default); a sweep keeps more streams than
        // that busy.  Read once, when the HIP runtime initialises - so this only helps before the first HIP call.
        if std::env::var_os("GPU_MAX_HW_QUEUES").is_none() {
            std::env::set_var("GPU_MAX_HW_QUEUES", "16");
        }
        let mut ctx = ptr::null_mut();
        let rc = unsafe { sys::ce_ctx_create(device, &mut ctx) };
        if rc != sys::CE_OK {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: last_error(ptr::null()) });
        }
        Ok(Self { ctx })
    }

    pub fn device_count() -> i32 {
        unsafe { sys::ce_device_count() }
    }

    fn check(&self, rc: i32, w: u32, h: u32, test_len: usize) -> Result<(), HipError> {
        match rc {
            sys::CE_OK => Ok(()),
            sys::CE_ERR_DIM_MISMATCH => Err(HipError::DimensionMismatch {
                expected: (w as usize, h as usize),
                actual: (if h > 0 { test_len / 3 / h as usize } else { 0 }, h as usize),
            }),
            _ => Err(HipError::MetricCalculation { metric: "hip".into(), reason: last_error(self.ctx) }),
        }
    }

    /// `calculate_metrics(&self, reference, test, width, height)` — one pair, host buffers.
    pub fn calculate_metrics(&mut self, reference: &[u8], test: &[u8], width: u32, height: u32, m: Metrics)
                             -> Result<Scores, HipError> {
        let mut s = sys::ce_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height,
                              m.mask(), m.flags(), sys::CE_DEFAULT_INTENSITY_TARGET, &mut s)
        };
        self.check(rc, width, height, test.len())?;
        Ok(s.into())
    }

    /// One pair of packed 16-bit RGB at its own precision (`ce_eval_pair_deep`): what a decoder hands over as
    /// `PixelData::Rgb16`, scored without `to_8bit`.  Sample `v` of a side of depth `d` (8, 10, 12 or 16) means the sRGB
    /// value `v / (2^d - 1)`; an 8-bit source widened to u16 goes in as depth 8.  PSNR is reported for equal depths only.
    pub fn calculate_metrics_deep(&mut self, reference: &[u16], ref_depth: u32, test: &[u16], test_depth: u32, width: u32,
                                  height: u32, m: Metrics) -> Result<Scores, HipError> {
        let mut s = sys::ce_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_deep(self.ctx, reference.as_ptr(), reference.len() * 2, ref_depth, test.as_ptr(), test.len() * 2,
                                   test_depth, width, height, m.mask(), m.flags(), sys::CE_DEFAULT_INTENSITY_TARGET, &mut s)
        };
        self.check(rc, width, height, test.len())?;  // three samples per pixel, as the bytes of an RGB8 image
        Ok(s.into())
    }

    /// One pair of packed f32 RGB in linear light with BT.709 / sRGB primaries (`ce_eval_pair_linear`): 1.0 is the white an
    /// 8-bit 255 maps to, values below 0 and above 1 are scored (HDR highlights, colours outside the sRGB gamut).  PSNR is not
    /// reported.  `intensity_target` is Butteraugli's: nits at 1.0.
    pub fn calculate_metrics_linear(&mut self, reference: &[f32], test: &[f32], width: u32, height: u32, m: Metrics,
                                    intensity_target: f32) -> Result<Scores, HipError> {
        let mut s = sys::ce_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_linear(self.ctx, reference.as_ptr(), reference.len() * 4, test.as_ptr(), test.len() * 4, width, height,
                                     m.mask(), m.flags(), intensity_target, &mut s)
        };
        self.check(rc, width, height, test.len())?;  // three samples per pixel, as the bytes of an RGB8 image
        Ok(s.into())
    }

    /// The whole `(codec, quality)` grid of `evaluate_image` (session.rs:375-376) in one call: decode every cell
    /// first, then pass `(reference, decoded, width, height)` per cell.  Cells that share a reference slice share
    /// one device slot.  Per-cell failures come back as `Err` in their position.
    pub fn evaluate_grid(&mut self, cells: &[(&[u8], &[u8], u32, u32)], m: Metrics) -> Result<Vec<Result<Scores, HipError>>, HipError> {
        let descs: Vec<sys::ce_pair_desc> = cells.iter().map(|(r, t, w, h)| sys::ce_pair_desc {
            reference: r.as_ptr(), reference_len: r.len(), test: t.as_ptr(), test_len: t.len(), width: *w, height: *h,
        }).collect();
        let mut out = vec![sys::ce_scores::default(); cells.len()];
        let rc = unsafe {
            sys::ce_eval_batch(self.ctx, descs.len(), descs.as_ptr(), m.mask(), m.flags(), sys::CE_DEFAULT_INTENSITY_TARGET,
                               out.as_mut_ptr())
        };
        if rc != sys::CE_OK {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: last_error(self.ctx) });
        }
        Ok(out.iter().zip(cells).map(|(s, (_, t, w, h))| self.check(s.status, *w, *h, t.len()).map(|_| (*s).into())).collect())
    }

    /// `xyb_roundtrip(rgb, width, height)` (src/metrics/xyb.rs:225-253), u8-exact.
    pub fn xyb_roundtrip(&mut self, rgb: &[u8], width: usize, height: usize) -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; rgb.len()];
        let rc = unsafe { sys::ce_xyb_roundtrip(self.ctx, rgb.as_ptr(), rgb.len(), width, height, out.as_mut_ptr()) };
        self.check(rc, width as u32, height as u32, rgb.len())?;
        Ok(out)
    }

    /// `compute_heuristics(rgb, width, height, _)` (crates/codec-compare/src/image_heuristics.rs:76-305) on the device;
    /// images under 3 x 3 are an error (the reference panics).
    pub fn compute_heuristics(&mut self, rgb: &[u8], width: usize, height: usize) -> Result<sys::ce_image_heuristics, HipError> {
        let mut out = sys::ce_image_heuristics::default();
        let rc = unsafe { sys::ce_image_heuristics_rgb8(self.ctx, rgb.as_ptr(), rgb.len(), width, height, &mut out) };
        self.check(rc, width as u32, height as u32, rgb.len())?;
        Ok(out)
    }

    /// One packed RGB8 image at the size a `ViewingCondition` displays it (`SimulationParams`, src/viewing.rs:308-331;
    /// `ce_resample_rgb8`): the fixed-point separable convolution of Pillow's `Image.resize`, bit for bit, on the device.
    pub fn resample_rgb8(&mut self, rgb: &[u8], width: u32, height: u32, out_width: u32, out_height: u32, filter: ResampleFilter)
                         -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; out_width as usize * out_height as usize * 3];
        let rc = unsafe {
            sys::ce_resample_rgb8(self.ctx, rgb.as_ptr(), rgb.len(), width, height, out_width, out_height, filter as i32,
                                  out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, rgb.len())?;
        Ok(out)
    }

    /// One packed `f32` RGB image in linear light at another size (`ce_resample_linear`): the convolution of Pillow's
    /// `Image.resize` on mode "F" images - f64 weights and accumulator, one rounding to f32 per pass - bit for bit, on the
    /// device, clamped to +-`CE_LINEAR_MAX`.  The lengths the library checks are in bytes.
    pub fn resample_linear(&mut self, rgb: &[f32], width: u32, height: u32, out_width: u32, out_height: u32, filter: ResampleFilter)
                           -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; out_width as usize * out_height as usize * 3];
        let rc = unsafe {
            sys::ce_resample_linear(self.ctx, rgb.as_ptr(), rgb.len() * 4, width, height, out_width, out_height, filter as i32,
                                    out.as_mut_ptr(), out.len() * 4)
        };
        self.check(rc, width, height, rgb.len())?;
        Ok(out)
    }

    /// A resident grid of `(reference, test)` pairs of one shape (`ce_batch_create`); `&self`, so that a source grid and
    /// the grids it is resampled into can live side by side (one call at a time per context, as everywhere).
    pub fn batch(&self, width: u32, height: u32, max_refs: u32, max_pairs: u32) -> Result<HipBatch<'_>, HipError> {
        let mut handle = std::ptr::null_mut();
        let rc = unsafe { sys::ce_batch_create(self.ctx, width, height, max_refs, max_pairs, &mut handle) };
        self.check(rc, width, height, 0)?;
        Ok(HipBatch { owner: self, handle, width, height })
    }

    /// `calculate_butteraugli_with_intensity` returning what `ButteraugliResult` holds (src/metrics/prelude.rs:64-65):
    /// the score and the per-pixel diffmap, row-major `width * height`, whose maximum is the score.
    pub fn calculate_butteraugli_with_diffmap(&mut self, reference: &[u8], test: &[u8], width: usize, height: usize,
                                              intensity_target: f32) -> Result<(f64, Vec<f32>), HipError> {
        let mut score = 0.0f64;
        let mut diffmap = vec![0.0f32; width * height];
        let rc = unsafe {
            sys::ce_calculate_butteraugli_diffmap(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width,
                                                  height, intensity_target, &mut score, diffmap.as_mut_ptr())
        };
        self.check(rc, width as u32, height as u32, test.len())?;
        Ok((score, diffmap))
    }

    /// `calculate_dssim` with the maps kept, the shape of dssim-core's `Dssim::compare` (`(Val, Vec<SsimMap>)`, which
    /// src/metrics/dssim.rs:68 drops): the score and one `SsimMap` per scale, level 0 at full resolution.
    pub fn calculate_dssim_with_ssim_maps(&mut self, reference: &[u8], test: &[u8], width: usize, height: usize)
                                          -> Result<(f64, Vec<SsimMap>), HipError> {
        let (mut n, mut lw, mut lh) = (0u32, [0u32; sys::CE_DSSIM_MAX_LEVELS], [0u32; sys::CE_DSSIM_MAX_LEVELS]);
        if width > 0 && height > 0 && width <= u32::MAX as usize && height <= u32::MAX as usize {
            unsafe { sys::ce_dssim_levels(width as u32, height as u32, &mut n, lw.as_mut_ptr(), lh.as_mut_ptr()) };
        }
        let sizes: Vec<(usize, usize)> = (0..n as usize).map(|l| (lw[l] as usize, lh[l] as usize)).collect();
        let mut maps = vec![0.0f32; sizes.iter().map(|(w, h)| w * h).sum()];
        let mut ssim = [0.0f64; sys::CE_DSSIM_MAX_LEVELS];
        let mut score = 0.0f64;
        let rc = unsafe {
            sys::ce_calculate_dssim_ssim_maps(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height,
                                              &mut score, ssim.as_mut_ptr(), maps.as_mut_ptr(), maps.len())
        };
        self.check(rc, width as u32, height as u32, test.len())?;
        let mut out = Vec::with_capacity(sizes.len());
        let mut off = 0;
        for (l, &(w, h)) in sizes.iter().enumerate() {
            out.push(SsimMap { width: w, height: h, map: maps[off..off + w * h].to_vec(), ssim: ssim[l] });
            off += w * h;
        }
        Ok((score, out))
    }

    /// `calculate_ssimulacra2` (src/metrics/ssimulacra2.rs:59) with everything the score pools kept: the score, the 108
    /// pooled features (`[scale][channel][6]`: mean and 4-norm of the SSIM, artifact and detail-lost maps; NaN past the
    /// image's scales) and one `Ssim2Maps` per scale, scale 0 at full resolution.
    pub fn calculate_ssimulacra2_with_maps(&mut self, reference: &[u8], test: &[u8], width: usize, height: usize)
                                           -> Result<(f64, [f64; sys::CE_SSIM2_MAX_SCALES * 18], Vec<Ssim2Maps>), HipError> {
        let (mut n, mut sw, mut sh) = (0u32, [0u32; sys::CE_SSIM2_MAX_SCALES], [0u32; sys::CE_SSIM2_MAX_SCALES]);
        if width > 0 && height > 0 && width <= u32::MAX as usize && height <= u32::MAX as usize {
            unsafe { sys::ce_ssimulacra2_scales(width as u32, height as u32, &mut n, sw.as_mut_ptr(), sh.as_mut_ptr()) };
        }
        let sizes: Vec<(usize, usize)> = (0..n as usize).map(|s| (sw[s] as usize, sh[s] as usize)).collect();
        let mut maps = vec![0.0f32; sizes.iter().map(|(w, h)| 9 * w * h).sum()];
        let mut features = [0.0f64; sys::CE_SSIM2_MAX_SCALES * 18];
        let mut score = 0.0f64;
        let rc = unsafe {
            sys::ce_calculate_ssimulacra2_maps(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width,
                                               height, &mut score, features.as_mut_ptr(), maps.as_mut_ptr(), maps.len())
        };
        self.check(rc, width as u32, height as u32, test.len())?;
        let mut out = Vec::with_capacity(sizes.len());
        let mut off = 0;
        for &(w, h) in &sizes {
            out.push(Ssim2Maps { width: w, height: h, maps: maps[off..off + 9 * w * h].to_vec() });
            off += 9 * w * h;
        }
        Ok((score, features, out))
    }
}

/// One scale of SSIMULACRA2's per-pixel error terms (ssim_map / edge_diff_map of the lineage behind
/// src/metrics/ssimulacra2.rs:96): `maps` is `[channel 3][kind 3][height][width]`, kinds `CE_SSIM2_MAP_SSIM`,
/// `CE_SSIM2_MAP_ARTIFACT`, `CE_SSIM2_MAP_DETAIL_LOST`.
#[derive(Clone, Debug)]
pub struct Ssim2Maps {
    pub width: usize,
    pub height: usize,
    pub maps: Vec<f32>,
}

/// dssim-core's `SsimMap` (re-exported at src/metrics/prelude.rs:45): one scale's per-pixel SSIM image, row-major
/// `width * height`, and that scale's pooled score.
#[derive(Clone, Debug)]
pub struct SsimMap {
    pub width: usize,
    pub height: usize,
    pub map: Vec<f32>,
    pub ssim: f64,
}

/// Page-locked host bytes (`ce_host_alloc`): a decoder that writes its RGB8 output here lets `evaluate_grid` copy it with
/// the DMA engines straight from this memory, overlapped with the kernels of the previous chunk, instead of staging it
/// through the library's ring with host threads.  Derefs to `[u8]`.
pub struct PinnedBytes {
    p: *mut u8,
    len: usize,
}

unsafe impl Send for PinnedBytes {}

impl HipMetrics {
    pub fn pinned(&self, len: usize) -> Result<PinnedBytes, HipError> {
        let mut p: *mut std::os::raw::c_void = ptr::null_mut();
        let rc = unsafe { sys::ce_host_alloc(self.ctx, len, &mut p) };
        if rc != sys::CE_OK {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: last_error(self.ctx) });
        }
        unsafe { ptr::write_bytes(p as *mut u8, 0, len) };
        Ok(PinnedBytes { p: p as *mut u8, len })
    }
}

impl std::ops::Deref for PinnedBytes {
    type Target = [u8];
    fn deref(&self) -> &[u8] {
        unsafe { std::slice::from_raw_parts(self.p, self.len) }
    }
}

impl std::ops::DerefMut for PinnedBytes {
    fn deref_mut(&mut self) -> &mut [u8] {
        unsafe { std::slice::from_raw_parts_mut(self.p, self.len) }
    }
}

impl Drop for PinnedBytes {
    fn drop(&mut self) {
        unsafe { sys::ce_host_free(ptr::null_mut(), self.p as *mut std::os::raw::c_void) }; // valid with or without its context
    }
}

impl Drop for HipMetrics {
    fn drop(&mut self) {
        unsafe { sys::ce_ctx_destroy(self.ctx) } // synchronises its streams first (the order gpu.rs:118-133 spells out)
    }
}

/// `Ssimulacra2Reference::{new, compare}`: the source image stays on the device with its reference-side state.
/// Must be dropped before the `HipMetrics` it was created from.
pub struct HipSsim2Reference<'a> {
    owner: &'a HipMetrics,
    handle: *mut sys::ce_ref,
    width: u32,
    height: u32,
}

impl<'a> HipSsim2Reference<'a> {
    pub fn new(owner: &'a HipMetrics, rgb: &[u8], width: u32, height: u32) -> Result<Self, HipError> {
        let mut handle = ptr::null_mut();
        let rc = unsafe { sys::ce_ref_create(owner.ctx, rgb.as_ptr(), rgb.len(), width, height, 0, &mut handle) };
        owner.check(rc, width, height, rgb.len())?;
        Ok(Self { owner, handle, width, height })
    }

    pub fn compare(&mut self, distorted: &[u8]) -> Result<f64, HipError> {
        let mut s = sys::ce_scores::default();
        let rc = unsafe {
            sys::ce_ref_compare(self.handle, distorted.as_ptr(), distorted.len(), sys::CE_METRIC_SSIMULACRA2,
                                sys::CE_DEFAULT_INTENSITY_TARGET, &mut s)
        };
        self.owner.check(rc, self.width, self.height, distorted.len())?;
        Ok(s.ssimulacra2)
    }

    /// The quality loop `for q in quality_levels { reference.compare(decoded[q]) }` (eval.rs:83-89) as one launch.
    pub fn compare_many(&mut self, distorted: &[&[u8]]) -> Result<Vec<f64>, HipError> {
        let ptrs: Vec<*const u8> = distorted.iter().map(|d| d.as_ptr()).collect();
        let lens: Vec<usize> = distorted.iter().map(|d| d.len()).collect();
        let mut out = vec![sys::ce_scores::default(); distorted.len()];
        let rc = unsafe {
            sys::ce_ref_compare_many(self.handle, ptrs.as_ptr(), lens.as_ptr(), distorted.len() as u32, sys::CE_METRIC_SSIMULACRA2,
                                     sys::CE_DEFAULT_INTENSITY_TARGET, out.as_mut_ptr())
        };
        self.owner.check(rc, self.width, self.height, 0)?;
        out.iter().zip(&lens).map(|(s, l)| self.owner.check(s.status, self.width, self.height, *l).map(|_| s.ssimulacra2)).collect()
    }
}

impl HipSsim2Reference<'_> {
    /// All metrics against the resident reference (the handle keeps every metric's reference-side state: XYB roundtrip,
    /// SSIMULACRA2 XYB pyramid, DSSIM img / mu / blur(img^2) pyramid, Butteraugli PsychoImage).  `scores[i].status`
    /// reports per-item failures.
    pub fn compare_many_metrics(&mut self, distorted: &[&[u8]], mask: u32, intensity_target: f32) -> Result<Vec<sys::ce_scores>, HipError> {
        let ptrs: Vec<*const u8> = distorted.iter().map(|d| d.as_ptr()).collect();
        let lens: Vec<usize> = distorted.iter().map(|d| d.len()).collect();
        let mut out = vec![sys::ce_scores::default(); distorted.len()];
        let rc = unsafe {
            sys::ce_ref_compare_many(self.handle, ptrs.as_ptr(), lens.as_ptr(), distorted.len() as u32, mask, intensity_target, out.as_mut_ptr())
        };
        self.owner.check(rc, self.width, self.height, 0)?;
        Ok(out)
    }

    /// `compute_heuristics` of the resident reference image: the heuristics CSV of a sweep without a second decode.
    pub fn heuristics(&mut self) -> Result<sys::ce_image_heuristics, HipError> {
        let mut out = sys::ce_image_heuristics::default();
        let rc = unsafe { sys::ce_ref_image_heuristics(self.handle, &mut out) };
        self.owner.check(rc, self.width, self.height, 0)?;
        Ok(out)
    }

    /// Compares so far that had to (re)build the reference side of (SSIMULACRA2, DSSIM, Butteraugli).
    pub fn reference_builds(&self) -> [u32; 3] {
        let mut b = [0u32; 3];
        unsafe { sys::ce_ref_stats(self.handle, b.as_mut_ptr()) };
        b
    }
}

impl Drop for HipSsim2Reference<'_> {
    fn drop(&mut self) {
        unsafe { sys::ce_ref_destroy(self.handle) }
    }
}

/// `GpuSsim2` look-alike for codec-iter's `Ssim2Backend` (eval.rs:56-92): `new(w, h)`, `compute(&mut self, ref, dis)`.
pub struct HipSsim2 {
    metrics: HipMetrics,
    width: u32,
    height: u32,
}

impl HipSsim2 {
    pub fn new(width: u32, height: u32) -> Result<Self, HipError> {
        Ok(Self { metrics: HipMetrics::new(0)?, width, height })
    }

    pub fn compute(&mut self, reference: &[u8], distorted: &[u8]) -> Result<f64, HipError> {
        let expected = self.width as usize * self.height as usize * 3;
        if reference.len() != expected || distorted.len() != expected {
            return Err(HipError::MetricCalculation {
                metric: "SSIMULACRA2".into(),
                reason: format!("Image size mismatch: expected {} bytes ({}x{}x3), got ref={} dis={}", expected, self.width,
                                self.height, reference.len(), distorted.len()),
            });
        }
        let m = Metrics { ssimulacra2: true, ..Metrics::default() };
        Ok(self.metrics.calculate_metrics(reference, distorted, self.width, self.height, m)?.ssimulacra2.unwrap_or(f64::NAN))
    }

    pub fn dimensions(&self) -> (u32, u32) {
        (self.width, self.height)
    }
}

fn last_error(ctx: *const sys::ce_ctx) -> String {
    let p = unsafe { sys::ce_last_error(ctx) };
    if p.is_null() { String::new() } else { unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned() }
}

/// `enum ce_resample_filter`: the kernel of `resample_rgb8` / `HipBatch::resample_pairs_into`.
#[derive(Debug, Clone, Copy, PartialEq, Eq, Default)]
#[repr(i32)]
pub enum ResampleFilter {
    Box = 0,
    Bilinear = 1,
    Bicubic = 2,
    #[default]
    Lanczos3 = 3,
}

/// A decoder's Y'CbCr planes in HOST memory (`ce_yuv_image` with `CE_MEM_HOST`): what a JPEG decoder in raw mode or dav1d
/// hands over.  `planes`: (Y, Cb, Cr), (Y, interleaved CbCr) with `semiplanar`, or (Y) for 4:0:0, each with its pitch in
/// bytes; bytes are u8 samples at depth 8 and little-endian u16 above.  The enum fields take the `sys::CE_YUV_*` /
/// `sys::CE_CHROMA_*` constants.  Device surfaces (rocJPEG / rocDecode) go through `sys::ce_yuv_image` directly.
#[derive(Debug, Clone, Copy)]
pub struct YuvPlanes<'p> {
    pub planes: [Option<(&'p [u8], usize)>; 3],
    pub subsampling: i32,
    pub semiplanar: bool,
    pub matrix: i32,
    pub range: i32,
    pub upsample: i32,
    pub depth: i32,
    pub msb_aligned: bool,
}

/// A gain map in host memory with its metadata (`ce_gainmap_image`, `ce_gainmap`): `samples` holds `height` rows of
/// `width * channels` bytes, `channels` 1 or 3, at most the base image's size.
#[derive(Clone, Copy, Debug)]
pub struct GainMap<'p> {
    pub samples: &'p [u8],
    pub width: u32,
    pub height: u32,
    pub channels: u32,
    pub metadata: sys::ce_gainmap,
}

impl GainMap<'_> {
    /// The C struct, after checking the slice's length: the struct carries none (the library checks the rest).
    fn to_sys(&self) -> Result<sys::ce_gainmap_image, HipError> {
        let want = self.width as usize * self.height as usize * self.channels as usize;
        if self.samples.len() != want {
            return Err(HipError::MetricCalculation {
                metric: "hip".into(),
                reason: format!("Invalid gain map size: expected {want} bytes, got {}", self.samples.len()),
            });
        }
        Ok(sys::ce_gainmap_image { samples: self.samples.as_ptr(), width: self.width, height: self.height, channels: self.channels })
    }
}

/// `ce_gainmap_weight`: W of a gain map's metadata, or `None` for metadata the library refuses.
pub fn gainmap_weight(metadata: &sys::ce_gainmap) -> Option<f64> {
    let mut w = 0f64;
    (unsafe { sys::ce_gainmap_weight(metadata, &mut w) } == sys::CE_OK).then_some(w)
}

/// `ce_gainmap_tables`: the log2-gain tables the kernel is handed, 256 per channel, or `None` for what the library refuses.
pub fn gainmap_tables(metadata: &sys::ce_gainmap, channels: u32) -> Option<Vec<f64>> {
    let mut out = vec![0f64; 256 * channels as usize];
    (unsafe { sys::ce_gainmap_tables(metadata, channels, out.as_mut_ptr(), out.len()) } == sys::CE_OK).then_some(out)
}

impl YuvPlanes<'_> {
    /// The C struct, after checking that every plane given holds `rows` rows of its pitch (the library checks the rest).
    fn to_sys(&self, width: u32, height: u32) -> Result<sys::ce_yuv_image, HipError> {
        let ch = if self.subsampling == sys::CE_YUV_420 { (height as usize + 1) / 2 } else { height as usize };
        let mut plane = [ptr::null::<std::os::raw::c_void>(); 3];
        let mut pitch = [0usize; 3];
        for (i, p) in self.planes.iter().enumerate() {
            if let Some((bytes, stride)) = p {
                let rows = if i == 0 { height as usize } else { ch };
                let bps = if self.depth == 8 { 1 } else { 2 };
                let cw = if self.subsampling == sys::CE_YUV_444 { width as usize } else { (width as usize + 1) / 2 };
                let row = bps * if i == 0 { width as usize } else if self.semiplanar { 2 * cw } else { cw };
                if rows > 0 && bytes.len() < (rows - 1) * stride + row {
                    return Err(HipError::MetricCalculation { metric: "hip".into(), reason: format!("Y'CbCr plane {i} is shorter than its rows") });
                }
                plane[i] = bytes.as_ptr().cast();
                pitch[i] = *stride;
            }
        }
        Ok(sys::ce_yuv_image {
            plane,
            pitch,
            subsampling: self.subsampling,
            layout: if self.semiplanar { sys::CE_YUV_SEMIPLANAR } else { sys::CE_YUV_PLANAR },
            matrix: self.matrix,
            range: self.range,
            upsample: self.upsample,
            depth: self.depth,
            msb_aligned: self.msb_aligned as i32,
            memory: sys::CE_MEM_HOST,
            lut: ptr::null(),
        })
    }
}

/// `ce_yuv_coefficients`: {KY, KRV, KGU, KGV, KBU, y0, c0} of the fixed-point conversion; `None` for a bad argument.
pub fn yuv_coefficients(matrix: i32, range: i32, depth_in: u32, depth_out: u32) -> Option<[i64; 7]> {
    let mut out = [0i64; 7];
    let rc = unsafe { sys::ce_yuv_coefficients(matrix, range, depth_in, depth_out, out.as_mut_ptr()) };
    (rc == sys::CE_OK).then_some(out)
}

impl HipMetrics {
    /// `ce_composite_rgba8`: straight-alpha RGBA8 source-over onto the opaque colour `bg` -> packed RGB8, on the device.
    pub fn composite_rgba8(&mut self, rgba: &[u8], width: u32, height: u32, bg: [u8; 3]) -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; width as usize * height as usize * 3];
        let rc = unsafe { sys::ce_composite_rgba8(self.ctx, rgba.as_ptr(), rgba.len(), width, height, bg.as_ptr(), out.as_mut_ptr(), out.len()) };
        self.check(rc, width, height, rgba.len())?;
        Ok(out)
    }

    /// `ce_composite_rgba16`: the same for u16 samples of `depth` bits (8, 10, 12 or 16) and a background at that depth.
    pub fn composite_rgba16(&mut self, rgba: &[u16], width: u32, height: u32, depth: u32, bg: [u16; 3]) -> Result<Vec<u16>, HipError> {
        let mut out = vec![0u16; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_composite_rgba16(self.ctx, rgba.as_ptr(), rgba.len(), width, height, depth, bg.as_ptr(), out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, rgba.len())?;
        Ok(out)
    }

    /// `ce_yuv_to_rgb8`: one image's planes -> packed RGB8, upsampled and converted on the device.
    pub fn yuv_to_rgb8(&mut self, image: &YuvPlanes<'_>, width: u32, height: u32) -> Result<Vec<u8>, HipError> {
        let c = image.to_sys(width, height)?;
        let mut out = vec![0u8; width as usize * height as usize * 3];
        let rc = unsafe { sys::ce_yuv_to_rgb8(self.ctx, &c, width, height, out.as_mut_ptr(), out.len()) };
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_yuv_to_linear`: one image's planes read by the colour description `colour` (H.273 primaries / transfer, the depth
    /// of the integer RGB grid, PQ's white) -> packed f32 RGB, linear light with sRGB primaries, in one kernel.
    pub fn yuv_to_linear(&mut self, image: &YuvPlanes<'_>, colour: &sys::ce_colour, width: u32, height: u32) -> Result<Vec<f32>, HipError> {
        let c = image.to_sys(width, height)?;
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe { sys::ce_yuv_to_linear(self.ctx, &c, colour, width, height, out.as_mut_ptr(), out.len()) };
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_cicp_over_to_linear`: `cicp_to_linear` of an RGBA image, blended in linear light over `background`.
    pub fn cicp_over_to_linear(&mut self, pixels: &[u8], format: i32, colour: &sys::ce_colour, width: u32, height: u32, background: [f32; 3])
                               -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_cicp_over_to_linear(self.ctx, pixels.as_ptr().cast(), pixels.len(), format, colour, width, height, background.as_ptr(),
                                        out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_hlg_over_to_linear`: `hlg_to_linear` of an RGBA image, blended in linear light over `background`.
    pub fn hlg_over_to_linear(&mut self, pixels: &[u8], format: i32, hlg: &sys::ce_hlg, width: u32, height: u32, background: [f32; 3])
                              -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_hlg_over_to_linear(self.ctx, pixels.as_ptr().cast(), pixels.len(), format, hlg, width, height, background.as_ptr(),
                                       out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_linear_over`: one float RGBA image in linear light, straight or premultiplied, over `background`.
    pub fn linear_over(&mut self, rgba: &[f32], premultiplied: bool, width: u32, height: u32, background: [f32; 3]) -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_linear_over(self.ctx, rgba.as_ptr().cast(), rgba.len() * 4, sys::CE_PIXEL_RGBA_F32, premultiplied as i32, width, height,
                                background.as_ptr(), out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, rgba.len() * 4)?;
        Ok(out)
    }

    /// `ce_hlg_to_linear`: one image of BT.2100 HLG code values (`format`: `sys::CE_PIXEL_RGB8` / `RGBA8` / `RGB16` / `RGBA16`;
    /// `pixels` are its bytes) read by `hlg` - primaries, depth, the display's peak and system gamma, the white that becomes
    /// 1.0 - -> packed f32 RGB, display light with sRGB primaries.
    pub fn hlg_to_linear(&mut self, pixels: &[u8], format: i32, hlg: &sys::ce_hlg, width: u32, height: u32) -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_hlg_to_linear(self.ctx, pixels.as_ptr().cast(), pixels.len(), format, hlg, width, height, out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_gainmap_to_linear`: one SDR base image (`format` and `pixels` as `hlg_to_linear`) read by `colour`, with the gain
    /// map `map` applied -> packed f32 RGB, the HDR rendition in linear light with sRGB primaries.
    pub fn gainmap_to_linear(&mut self, pixels: &[u8], format: i32, colour: &sys::ce_colour, map: &GainMap<'_>, width: u32, height: u32)
                             -> Result<Vec<f32>, HipError> {
        let image = map.to_sys()?;
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_gainmap_to_linear(self.ctx, pixels.as_ptr().cast(), pixels.len(), format, colour, &image, &map.metadata, width, height,
                                      out.as_mut_ptr(), out.len())
        };
        self.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_tensor_to_rgb8`: image 0 of a strided tensor as an RGB8 slot would hold it.
    ///
    /// # Safety
    /// `t.data` and its strides must describe memory of the kind `t.memory` names that holds every element of a
    /// `width` x `height` image of three channels.
    pub unsafe fn tensor_to_rgb8(&mut self, t: &sys::ce_tensor_image, width: u32, height: u32) -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; width as usize * height as usize * 3];
        let rc = sys::ce_tensor_to_rgb8(self.ctx, t, width, height, out.as_mut_ptr(), out.len());
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_tensor_to_rgb16`: the same as a deep side of `depth_out` bits (8, 10, 12 or 16) would hold it.
    ///
    /// # Safety
    /// As `tensor_to_rgb8`.
    pub unsafe fn tensor_to_rgb16(&mut self, t: &sys::ce_tensor_image, width: u32, height: u32, depth_out: u32) -> Result<Vec<u16>, HipError> {
        let mut out = vec![0u16; width as usize * height as usize * 3];
        let rc = sys::ce_tensor_to_rgb16(self.ctx, t, width, height, depth_out, out.as_mut_ptr(), out.len());
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_tensor_to_linear`: a float tensor as a slot of a linear batch would hold it.
    ///
    /// # Safety
    /// As `tensor_to_rgb8`.
    pub unsafe fn tensor_to_linear(&mut self, t: &sys::ce_tensor_image, width: u32, height: u32) -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = sys::ce_tensor_to_linear(self.ctx, t, width, height, out.as_mut_ptr(), out.len());
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_yuv_hlg_to_linear`: one image's planes in HLG, in one kernel (`hlg.depth` is the integer RGB grid's, >= the samples').
    pub fn yuv_hlg_to_linear(&mut self, image: &YuvPlanes<'_>, hlg: &sys::ce_hlg, width: u32, height: u32) -> Result<Vec<f32>, HipError> {
        let c = image.to_sys(width, height)?;
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe { sys::ce_yuv_hlg_to_linear(self.ctx, &c, hlg, width, height, out.as_mut_ptr(), out.len()) };
        self.check(rc, width, height, out.len())?;
        Ok(out)
    }

    /// `ce_eval_pair_hdr_fidelity`: PSNR in the PQ domain and BT.2124's Delta E ITP of one pair of packed f32 RGB, linear light
    /// with sRGB primaries; `depth` (10, 12 or 16) is the PQ code grid, `white_nits` the luminance of sample value 1.0.
    pub fn hdr_fidelity(&mut self, reference: &[f32], test: &[f32], width: u32, height: u32, depth: u32, white_nits: f32)
                        -> Result<sys::ce_hdr_scores, HipError> {
        let mut out = sys::ce_hdr_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_hdr_fidelity(self.ctx, reference.as_ptr(), reference.len() * 4, test.as_ptr(), test.len() * 4, width, height,
                                           depth, white_nits, &mut out)
        };
        self.check(rc, width, height, test.len() * 4)?;
        Ok(out)
    }

    /// `ce_eval_pair_msssim`: SSIM (`levels` 1) and MS-SSIM (5) of one pair of packed RGB8 on the encoded sample values.
    pub fn ms_ssim(&mut self, reference: &[u8], test: &[u8], width: u32, height: u32, levels: u32) -> Result<sys::ce_msssim_scores, HipError> {
        let mut out = sys::ce_msssim_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_msssim(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height, levels, &mut out)
        };
        self.check(rc, width, height, test.len())?;
        Ok(out)
    }

    /// `ce_eval_pair_msssim_deep`: the same for packed u16 RGB of `depth` bits (8, 10, 12 or 16) on both sides.
    pub fn ms_ssim_deep(&mut self, reference: &[u16], test: &[u16], depth: u32, width: u32, height: u32, levels: u32)
                        -> Result<sys::ce_msssim_scores, HipError> {
        let mut out = sys::ce_msssim_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_msssim_deep(self.ctx, reference.as_ptr(), reference.len() * 2, test.as_ptr(), test.len() * 2, depth, width,
                                          height, levels, &mut out)
        };
        self.check(rc, width, height, test.len() * 2)?;
        Ok(out)
    }

    /// `ce_eval_pair_ciede2000`: CIEDE2000 of one pair of packed RGB8 read as sRGB; `thresholds_q20` (at most eight, in units of
    /// 2^-20) are what `n_above` counts the pixels above.
    pub fn ciede2000(&mut self, reference: &[u8], test: &[u8], width: u32, height: u32, thresholds_q20: &[u32])
                     -> Result<sys::ce_ciede2000_scores, HipError> {
        let mut out = sys::ce_ciede2000_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_ciede2000(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height,
                                        thresholds_q20.as_ptr(), thresholds_q20.len() as u32, &mut out)
        };
        self.check(rc, width, height, test.len())?;
        Ok(out)
    }

    /// `ce_eval_pair_ciede2000_deep`: the same for packed u16 RGB, the reference at `ref_depth` and the test at `test_depth` bits
    /// (each 8, 10, 12 or 16).
    pub fn ciede2000_deep(&mut self, reference: &[u16], test: &[u16], ref_depth: u32, test_depth: u32, width: u32, height: u32,
                          thresholds_q20: &[u32]) -> Result<sys::ce_ciede2000_scores, HipError> {
        let mut out = sys::ce_ciede2000_scores::default();
        let rc = unsafe {
            sys::ce_eval_pair_ciede2000_deep(self.ctx, reference.as_ptr(), reference.len() * 2, test.as_ptr(), test.len() * 2, ref_depth,
                                             test_depth, width, height, thresholds_q20.as_ptr(), thresholds_q20.len() as u32, &mut out)
        };
        self.check(rc, width, height, test.len() * 2)?;
        Ok(out)
    }

    /// `ce_eval_pair_ciede2000_map`: where one pair of packed RGB8 read as sRGB differs, and in which direction of colour space -
    /// see `HipBatch::ciede2000_map`.
    pub fn ciede2000_map(&mut self, reference: &[u8], test: &[u8], width: u32, height: u32, what: u32, block: u32, want_map: bool,
                         thresholds_q20: &[u32]) -> Result<Ciede2000Maps, HipError> {
        let mut out = Ciede2000Maps::sized(1, width, height, block, want_map, thresholds_q20.len());
        let rc = unsafe {
            sys::ce_eval_pair_ciede2000_map(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height, what,
                                            block, out.map_ptr(), out.map.len(), slice_or_null(thresholds_q20),
                                            thresholds_q20.len() as u32, out.over_ptr())
        };
        self.check(rc, width, height, test.len())?;
        Ok(out)
    }

    /// `ce_eval_pair_ciede2000_map_deep`: the same for packed u16 RGB, the reference at `ref_depth` and the test at `test_depth`
    /// bits (each 8, 10, 12 or 16).
    pub fn ciede2000_map_deep(&mut self, reference: &[u16], test: &[u16], ref_depth: u32, test_depth: u32, width: u32, height: u32,
                              what: u32, block: u32, want_map: bool, thresholds_q20: &[u32]) -> Result<Ciede2000Maps, HipError> {
        let mut out = Ciede2000Maps::sized(1, width, height, block, want_map, thresholds_q20.len());
        let rc = unsafe {
            sys::ce_eval_pair_ciede2000_map_deep(self.ctx, reference.as_ptr(), reference.len() * 2, test.as_ptr(), test.len() * 2, ref_depth,
                                                 test_depth, width, height, what, block, out.map_ptr(), out.map.len(),
                                                 slice_or_null(thresholds_q20), thresholds_q20.len() as u32, out.over_ptr())
        };
        self.check(rc, width, height, test.len() * 2)?;
        Ok(out)
    }

    /// `ce_eval_pair_msssim_map`: where one pair of packed RGB8 differs at `level` - see `HipBatch::ms_ssim_map`.
    pub fn ms_ssim_map(&mut self, reference: &[u8], test: &[u8], width: u32, height: u32, levels: u32, level: u32, what: u32, block: u32,
                       want_map: bool, thresholds_q32: &[u32]) -> Result<MsSsimMaps, HipError> {
        let mut out = MsSsimMaps::sized(1, width, height, levels, level, block, want_map, thresholds_q32.len());
        let rc = unsafe {
            sys::ce_eval_pair_msssim_map(self.ctx, reference.as_ptr(), reference.len(), test.as_ptr(), test.len(), width, height, levels, level,
                                         what, block, out.map_ptr(), out.map.len(), slice_or_null(thresholds_q32),
                                         thresholds_q32.len() as u32, out.over_ptr())
        };
        self.check(rc, width, height, test.len())?;
        Ok(out)
    }

    /// `ce_eval_pair_msssim_map_deep`: the same for packed u16 RGB of `depth` bits (8, 10, 12 or 16) on both sides.
    pub fn ms_ssim_map_deep(&mut self, reference: &[u16], test: &[u16], depth: u32, width: u32, height: u32, levels: u32, level: u32,
                            what: u32, block: u32, want_map: bool, thresholds_q32: &[u32]) -> Result<MsSsimMaps, HipError> {
        let mut out = MsSsimMaps::sized(1, width, height, levels, level, block, want_map, thresholds_q32.len());
        let rc = unsafe {
            sys::ce_eval_pair_msssim_map_deep(self.ctx, reference.as_ptr(), reference.len() * 2, test.as_ptr(), test.len() * 2, depth, width,
                                              height, levels, level, what, block, out.map_ptr(), out.map.len(),
                                              slice_or_null(thresholds_q32), thresholds_q32.len() as u32, out.over_ptr())
        };
        self.check(rc, width, height, test.len() * 2)?;
        Ok(out)
    }

    /// `ce_yuv_plane_fidelity`: PSNR (`levels` 0), + SSIM (1), + MS-SSIM (5) of host Y'CbCr images plane by plane, on the planes
    /// as a decoder wrote them: `tests[i]` against `refs[pair_ref[i]]`, or against `refs[i]` without a pair table.  Every image is
    /// `width` x `height` with one subsampling and one depth.  Device surfaces go through `sys::ce_yuv_plane_fidelity` directly.
    pub fn plane_fidelity(&mut self, refs: &[YuvPlanes<'_>], tests: &[YuvPlanes<'_>], width: u32, height: u32, pair_ref: Option<&[u32]>,
                          levels: u32) -> Result<Vec<sys::ce_plane_scores>, HipError> {
        if pair_ref.is_some_and(|t| t.len() != tests.len()) {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "the pair table names another number of pairs than there are tests".into() });
        }
        let r = refs.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let t = tests.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let mut out = vec![sys::ce_plane_scores::default(); tests.len()];
        let rc = unsafe {
            sys::ce_yuv_plane_fidelity(self.ctx, width, height, r.as_ptr(), r.len() as u32, t.as_ptr(), t.len() as u32,
                                       pair_ref.map_or(ptr::null(), |p| p.as_ptr()), levels, out.as_mut_ptr())
        };
        self.check(rc, width, height, 0)?;
        Ok(out)
    }

    /// `ce_yuv_plane_hvs`: PSNR-HVS and PSNR-HVS-M of host Y'CbCr images plane by plane, with `plane_fidelity`'s images and pair
    /// table; `step` is the samples from an 8 x 8 DCT block to the next, 1 to 8.  Device surfaces go through
    /// `sys::ce_yuv_plane_hvs` directly.
    pub fn plane_hvs(&mut self, refs: &[YuvPlanes<'_>], tests: &[YuvPlanes<'_>], width: u32, height: u32, pair_ref: Option<&[u32]>,
                     step: u32) -> Result<Vec<sys::ce_plane_hvs_scores>, HipError> {
        if pair_ref.is_some_and(|t| t.len() != tests.len()) {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "the pair table names another number of pairs than there are tests".into() });
        }
        let r = refs.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let t = tests.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let mut out = vec![sys::ce_plane_hvs_scores::default(); tests.len()];
        let rc = unsafe {
            sys::ce_yuv_plane_hvs(self.ctx, width, height, r.as_ptr(), r.len() as u32, t.as_ptr(), t.len() as u32,
                                  pair_ref.map_or(ptr::null(), |p| p.as_ptr()), step, out.as_mut_ptr())
        };
        self.check(rc, width, height, 0)?;
        Ok(out)
    }

    /// `ce_yuv_plane_vif`: pixel-domain VIF (VIFp) of host Y'CbCr images plane by plane, with `plane_fidelity`'s images and pair
    /// table; a plane needs 41 x 41 samples to run and luma must.  Device surfaces go through `sys::ce_yuv_plane_vif` directly.
    pub fn plane_vif(&mut self, refs: &[YuvPlanes<'_>], tests: &[YuvPlanes<'_>], width: u32, height: u32,
                     pair_ref: Option<&[u32]>) -> Result<Vec<sys::ce_plane_vif_scores>, HipError> {
        if pair_ref.is_some_and(|t| t.len() != tests.len()) {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "the pair table names another number of pairs than there are tests".into() });
        }
        let r = refs.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let t = tests.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let mut out = vec![sys::ce_plane_vif_scores::default(); tests.len()];
        let rc = unsafe {
            sys::ce_yuv_plane_vif(self.ctx, width, height, r.as_ptr(), r.len() as u32, t.as_ptr(), t.len() as u32,
                                  pair_ref.map_or(ptr::null(), |p| p.as_ptr()), out.as_mut_ptr())
        };
        self.check(rc, width, height, 0)?;
        Ok(out)
    }

    /// `ce_yuv_plane_gmsd`: GMSD (gradient magnitude similarity deviation) and its mean of host Y'CbCr images plane by plane, with
    /// `plane_fidelity`'s images and pair table; every plane of any size runs.  `sum_q2[p]` is [low 64 bits, high 64 bits]:
    /// `(hi as u128) << 64 | lo as u128` is the sum of squares.  Device surfaces go through `sys::ce_yuv_plane_gmsd` directly.
    pub fn plane_gmsd(&mut self, refs: &[YuvPlanes<'_>], tests: &[YuvPlanes<'_>], width: u32, height: u32,
                      pair_ref: Option<&[u32]>) -> Result<Vec<sys::ce_plane_gmsd_scores>, HipError> {
        if pair_ref.is_some_and(|t| t.len() != tests.len()) {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "the pair table names another number of pairs than there are tests".into() });
        }
        let r = refs.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let t = tests.iter().map(|p| p.to_sys(width, height)).collect::<Result<Vec<_>, _>>()?;
        let mut out = vec![sys::ce_plane_gmsd_scores::default(); tests.len()];
        let rc = unsafe {
            sys::ce_yuv_plane_gmsd(self.ctx, width, height, r.as_ptr(), r.len() as u32, t.as_ptr(), t.len() as u32,
                                   pair_ref.map_or(ptr::null(), |p| p.as_ptr()), out.as_mut_ptr())
        };
        self.check(rc, width, height, 0)?;
        Ok(out)
    }

    /// `ce_eval_pair_delta_e_itp_map`: where one pair of packed f32 RGB differs - see `HipBatch::delta_e_itp_map`.
    pub fn delta_e_itp_map(&mut self, reference: &[f32], test: &[f32], width: u32, height: u32, depth: u32, white_nits: f32, block: u32,
                           want_map: bool, thresholds_q20: &[u32]) -> Result<DeltaEItpMaps, HipError> {
        let mut out = DeltaEItpMaps::sized(1, width, height, block, want_map, thresholds_q20.len());
        let rc = unsafe {
            sys::ce_eval_pair_delta_e_itp_map(self.ctx, reference.as_ptr(), reference.len() * 4, test.as_ptr(), test.len() * 4, width, height,
                                              depth, white_nits, block, out.map_ptr(), out.map.len(), slice_or_null(thresholds_q20),
                                              thresholds_q20.len() as u32, out.over_ptr())
        };
        self.check(rc, width, height, test.len() * 4)?;
        Ok(out)
    }
}

/// What `ce_batch_delta_e_itp_map` returns: per pair the BT.2124 Delta E ITP of every pixel in units of 2^-20
/// (`sys::CE_DELTA_E_ITP_Q20` is 1.0), saturated at `u32::MAX` - or at `block` 2 ..= 64 the maximum of each block x block cell -
/// as `[count][cells_h][cells_w]`, empty when no map was asked for; and `[count][n_thresholds]` counts of the pixels above each
/// threshold, empty without thresholds.
pub struct DeltaEItpMaps {
    pub map: Vec<u32>,
    pub cells_w: u32,
    pub cells_h: u32,
    pub over: Vec<u64>,
}

impl DeltaEItpMaps {
    fn sized(count: u32, width: u32, height: u32, block: u32, want_map: bool, n_thresholds: usize) -> Self {
        let b = block.max(1);
        let (cells_w, cells_h) = ((width + b - 1) / b, (height + b - 1) / b);
        let n = if want_map { count as usize * cells_w as usize * cells_h as usize } else { 0 };
        DeltaEItpMaps { map: vec![0u32; n], cells_w, cells_h, over: vec![0u64; count as usize * n_thresholds] }
    }
    fn map_ptr(&mut self) -> *mut u32 {
        if self.map.is_empty() { std::ptr::null_mut() } else { self.map.as_mut_ptr() }
    }
    fn over_ptr(&mut self) -> *mut u64 {
        if self.over.is_empty() { std::ptr::null_mut() } else { self.over.as_mut_ptr() }
    }
}

/// What `ce_batch_ciede2000_map` returns: per pair one of a pixel's four values in units of 2^-20 (`sys::CE_CIEDE2000_Q20` is
/// 1.0) - the Delta E 2000 itself or the magnitude of its lightness, chroma or hue term, which may exceed the Delta E - or at
/// `block` 2 ..= 64 the maximum of each block x block cell - as `[count][cells_h][cells_w]`, empty when no map was asked for; and
/// `[count][n_thresholds]` counts of the pixels above each threshold, empty without thresholds.
pub struct Ciede2000Maps {
    pub map: Vec<u32>,
    pub cells_w: u32,
    pub cells_h: u32,
    pub over: Vec<u64>,
}

impl Ciede2000Maps {
    fn sized(count: u32, width: u32, height: u32, block: u32, want_map: bool, n_thresholds: usize) -> Self {
        let b = block.max(1);
        let (cells_w, cells_h) = ((width + b - 1) / b, (height + b - 1) / b);
        let n = if want_map { count as usize * cells_w as usize * cells_h as usize } else { 0 };
        Ciede2000Maps { map: vec![0u32; n], cells_w, cells_h, over: vec![0u64; count as usize * n_thresholds] }
    }
    fn map_ptr(&mut self) -> *mut u32 {
        if self.map.is_empty() { std::ptr::null_mut() } else { self.map.as_mut_ptr() }
    }
    fn over_ptr(&mut self) -> *mut u64 {
        if self.over.is_empty() { std::ptr::null_mut() } else { self.over.as_mut_ptr() }
    }
}

/// What `ce_batch_msssim_map` returns: per pair and channel every valid position's `2^32 - q` in units of 2^-32
/// (`sys::CE_MSSSIM_Q32` is an SSIM of 1.0), `q` the integer `ms_ssim` sums, saturated to `[0, u32::MAX]` - or at `block` 2 ..= 64
/// the maximum of each block x block cell - as `[count][3][cells_h][cells_w]`, empty when no map was asked for; and
/// `[count][3][n_thresholds]` counts of the positions above each threshold, empty without thresholds.  What the library refuses
/// (`levels`, `level`, an image too small) leaves the map empty for it to refuse.
pub struct MsSsimMaps {
    pub map: Vec<u32>,
    pub cells_w: u32,
    pub cells_h: u32,
    pub over: Vec<u64>,
}

impl MsSsimMaps {
    fn sized(count: u32, width: u32, height: u32, levels: u32, level: u32, block: u32, want_map: bool, n_thresholds: usize) -> Self {
        let b = block.max(1);
        let (cells_w, cells_h) = match msssim_levels(width, height, levels) {
            Some(lv) if (level as usize) < lv.len() => ((lv[level as usize].0 - 10 + b - 1) / b, (lv[level as usize].1 - 10 + b - 1) / b),
            _ => (0, 0),
        };
        let n = if want_map { count as usize * 3 * cells_w as usize * cells_h as usize } else { 0 };
        MsSsimMaps { map: vec![0u32; n], cells_w, cells_h, over: vec![0u64; count as usize * 3 * n_thresholds] }
    }
    fn map_ptr(&mut self) -> *mut u32 {
        if self.map.is_empty() { std::ptr::null_mut() } else { self.map.as_mut_ptr() }
    }
    fn over_ptr(&mut self) -> *mut u64 {
        if self.over.is_empty() { std::ptr::null_mut() } else { self.over.as_mut_ptr() }
    }
}

fn slice_or_null(s: &[u32]) -> *const u32 {
    if s.is_empty() { std::ptr::null() } else { s.as_ptr() }
}

/// `ce_pq_code_thresholds`: the decision thresholds of PQ code values on linear light, `T[1 ..= 2^depth - 1]`; a pure host
/// function.  `None` for a depth other than 10, 12 or 16 or a `white_nits` that is not finite and > 0.
pub fn pq_code_thresholds(depth: u32, white_nits: f32) -> Option<Vec<f32>> {
    if !matches!(depth, 10 | 12 | 16) {
        return None;
    }
    let mut out = vec![0f32; (1usize << depth) - 1];
    let rc = unsafe { sys::ce_pq_code_thresholds(depth, white_nits, out.as_mut_ptr(), out.len()) };
    (rc == sys::CE_OK).then_some(out)
}

/// `ce_vif_window`: the 17, 9, 5 or 3 literals of the window of VIFp's scale 1 .. 4 (empty for another scale); a pure host
/// function.
pub fn vif_window(scale: u32) -> Vec<f64> {
    let mut g = [0.0f64; 17];
    if unsafe { sys::ce_vif_window(scale, g.as_mut_ptr()) } != sys::CE_OK {
        return Vec::new();
    }
    g[..[17, 9, 5, 3][scale as usize - 1]].to_vec()
}

/// `ce_msssim_window`: the eleven literals of the SSIM / MS-SSIM window; a pure host function.
pub fn msssim_window() -> [f64; 11] {
    let mut g = [0f64; 11];
    unsafe { sys::ce_msssim_window(g.as_mut_ptr()) };
    g
}

/// `ce_ciede2000_pixels`: the per-pixel CIEDE2000 in units of 2^-20 of packed u16 RGB at `ref_depth` / `test_depth` bits - the
/// kernel's pixel text compiled for the host; `None` for sides of unequal length, a length that is no multiple of 3 or a depth
/// that is none of 8, 10, 12, 16.  A pure host function.
pub fn ciede2000_pixels(reference: &[u16], ref_depth: u32, test: &[u16], test_depth: u32) -> Option<Vec<u32>> {
    if reference.len() != test.len() || reference.len() % 3 != 0 {
        return None;
    }
    let mut out = vec![0u32; reference.len() / 3];
    let rc = unsafe { sys::ce_ciede2000_pixels(reference.as_ptr(), ref_depth, test.as_ptr(), test_depth, out.len(), out.as_mut_ptr()) };
    (rc == sys::CE_OK).then_some(out)
}

/// `ce_ciede2000_pixel_terms`: the four per-pixel values of the CIEDE2000 maps in units of 2^-20, `[n][4]` indexed by
/// `sys::CE_CIEDE2000_MAP_DE`, `_DL`, `_DC`, `_DH` - column 0 is `ciede2000_pixels`' value; `None` as there.  A pure host function.
pub fn ciede2000_pixel_terms(reference: &[u16], ref_depth: u32, test: &[u16], test_depth: u32) -> Option<Vec<[u32; 4]>> {
    if reference.len() != test.len() || reference.len() % 3 != 0 {
        return None;
    }
    let mut out = vec![[0u32; 4]; reference.len() / 3];
    let rc = unsafe {
        sys::ce_ciede2000_pixel_terms(reference.as_ptr(), ref_depth, test.as_ptr(), test_depth, out.len(), out.as_mut_ptr() as *mut u32)
    };
    (rc == sys::CE_OK).then_some(out)
}

/// `ce_msssim_levels`: the (width, height) of every level of SSIM (`levels` 1) or MS-SSIM (5) on a width x height image; `None`
/// for other `levels` and for an image too small.  A pure host function.
pub fn msssim_levels(width: u32, height: u32, levels: u32) -> Option<Vec<(u32, u32)>> {
    let (mut n, mut w, mut h) = (0u32, [0u32; 5], [0u32; 5]);
    let rc = unsafe { sys::ce_msssim_levels(width, height, levels, &mut n, w.as_mut_ptr(), h.as_mut_ptr()) };
    (rc == sys::CE_OK).then(|| (0..n as usize).map(|l| (w[l], h[l])).collect())
}

/// `ce_hdr_fidelity_matrices`: the two row-major 3 x 3 matrices the HDR fidelity kernel is handed - BT.2020 <- sRGB primaries,
/// and BT.2100's LMS <- BT.2020.
pub fn hdr_fidelity_matrices() -> ([f32; 9], [f32; 9]) {
    let (mut a, mut b) = ([0f32; 9], [0f32; 9]);
    unsafe { sys::ce_hdr_fidelity_matrices(a.as_mut_ptr(), b.as_mut_ptr()) };
    (a, b)
}

/// `ce_icc_describe`: what the library's parser reads from an ICC profile, without a device.  `kind` is
/// `sys::CE_ICC_SUPPORTED` for the matrix/TRC profiles `HipIccProfile` takes.
pub fn icc_describe(profile: &[u8]) -> sys::ce_icc_description {
    let mut d: sys::ce_icc_description = unsafe { std::mem::zeroed() };
    unsafe { sys::ce_icc_describe(profile.as_ptr(), profile.len(), &mut d) };
    d
}

/// `ce_icc_lut_describe`: what the library's parser reads from a LUT-based ICC profile, without a device.  `kind` is
/// `sys::CE_ICC_LUT_SUPPORTED` for the profiles `HipIccProfile::new_lut` takes.
pub fn icc_lut_describe(profile: &[u8], intent: i32) -> sys::ce_icc_lut_description {
    let mut d: sys::ce_icc_lut_description = unsafe { std::mem::zeroed() };
    unsafe { sys::ce_icc_lut_describe(profile.as_ptr(), profile.len(), intent, &mut d) };
    d
}

/// `ce_icc`: a matrix/TRC ICC profile applied on the device, parsed by the library itself (no CMS).  A LUT-based, Gray, CMYK
/// or malformed profile is refused with the reason; those keep the colour-table route (`ce_lut_*`).
pub struct HipIccProfile<'a> {
    owner: &'a HipMetrics,
    handle: *mut sys::ce_icc,
}

impl<'a> HipIccProfile<'a> {
    pub fn new(owner: &'a HipMetrics, profile: &[u8]) -> Result<Self, HipError> {
        let mut handle = ptr::null_mut();
        let rc = unsafe { sys::ce_icc_create(owner.ctx, profile.as_ptr(), profile.len(), &mut handle) };
        owner.check(rc, 0, 0, 0)?;
        Ok(Self { owner, handle })
    }

    /// `ce_icc_lut_create`: the same handle for a LUT-based profile (an A2B tag of type mAB, mft2 or mft1),
    /// evaluated from the profile itself.  `intent` 0, 1 or 2 chooses A2B0 / A2B1 / A2B2; `interpolation` is
    /// `sys::CE_ICC_CLUT_TRILINEAR` or `sys::CE_ICC_CLUT_TETRAHEDRAL`.  Every call that takes a `HipIccProfile` takes it.
    pub fn new_lut(owner: &'a HipMetrics, profile: &[u8], intent: i32, interpolation: i32) -> Result<Self, HipError> {
        let mut handle = ptr::null_mut();
        let rc = unsafe { sys::ce_icc_lut_create(owner.ctx, profile.as_ptr(), profile.len(), intent, interpolation, &mut handle) };
        owner.check(rc, 0, 0, 0)?;
        Ok(Self { owner, handle })
    }

    /// `ce_icc_over_to_linear`: `to_linear` of an RGBA image, blended in linear light over `background`.
    pub fn over_to_linear(&self, pixels: &[u8], format: i32, depth: u32, width: u32, height: u32, background: [f32; 3])
                          -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_icc_over_to_linear(self.owner.ctx, pixels.as_ptr().cast(), pixels.len(), format, depth, self.handle, width, height,
                                       background.as_ptr(), out.as_mut_ptr(), out.len())
        };
        self.owner.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_icc_to_linear`: one image (`format` and `pixels` as `hlg_to_linear`, samples of `depth` bits) -> packed f32 RGB,
    /// linear light with sRGB primaries.
    pub fn to_linear(&self, pixels: &[u8], format: i32, depth: u32, width: u32, height: u32) -> Result<Vec<f32>, HipError> {
        let mut out = vec![0f32; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_icc_to_linear(self.owner.ctx, pixels.as_ptr().cast(), pixels.len(), format, depth, self.handle, width, height,
                                  out.as_mut_ptr(), out.len())
        };
        self.owner.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_icc_to_srgb8`: the same image as packed sRGB8, what `transform_to_srgb` (src/metrics/icc.rs:69-103) returns.
    pub fn to_srgb8(&self, pixels: &[u8], format: i32, depth: u32, width: u32, height: u32) -> Result<Vec<u8>, HipError> {
        let mut out = vec![0u8; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_icc_to_srgb8(self.owner.ctx, pixels.as_ptr().cast(), pixels.len(), format, depth, self.handle, width, height,
                                 out.as_mut_ptr(), out.len())
        };
        self.owner.check(rc, width, height, pixels.len())?;
        Ok(out)
    }

    /// `ce_icc_to_srgb16`: the same image as packed u16 sRGB code values of `depth_out` bits (8, 10, 12 or 16).
    pub fn to_srgb16(&self, pixels: &[u8], format: i32, depth: u32, width: u32, height: u32, depth_out: u32) -> Result<Vec<u16>, HipError> {
        let mut out = vec![0u16; width as usize * height as usize * 3];
        let rc = unsafe {
            sys::ce_icc_to_srgb16(self.owner.ctx, pixels.as_ptr().cast(), pixels.len(), format, depth, self.handle, width, height, depth_out,
                                  out.as_mut_ptr(), out.len())
        };
        self.owner.check(rc, width, height, pixels.len())?;
        Ok(out)
    }
}

impl Drop for HipIccProfile<'_> {
    fn drop(&mut self) {
        unsafe { sys::ce_icc_destroy(self.handle) };
    }
}

/// `ce_batch`: images of one shape resident on the device, scored in one launch.  Resampling one grid into another
/// (`resample_pairs_into`) scores a sweep at the size a `ViewingCondition` displays it (src/viewing.rs:244-301) without
/// another upload.
pub struct HipBatch<'a> {
    owner: &'a HipMetrics,
    handle: *mut sys::ce_batch,
    width: u32,
    height: u32,
}

impl HipBatch<'_> {
    fn check(&self, rc: i32, len: usize) -> Result<(), HipError> {
        self.owner.check(rc, self.width, self.height, len)
    }

    pub fn set_reference(&mut self, ref_index: u32, rgb: &[u8]) -> Result<(), HipError> {
        let rc = unsafe { sys::ce_batch_set_reference(self.handle, ref_index, rgb.as_ptr(), rgb.len()) };
        self.check(rc, rgb.len())
    }

    pub fn set_test(&mut self, pair_index: u32, ref_index: u32, rgb: &[u8]) -> Result<(), HipError> {
        let rc = unsafe { sys::ce_batch_set_test(self.handle, pair_index, ref_index, rgb.as_ptr(), rgb.len()) };
        self.check(rc, rgb.len())
    }

    /// `ce_batch_set_reference_over`: one straight-alpha RGBA image (`format`: `sys::CE_PIXEL_RGBA8`, or
    /// `sys::CE_PIXEL_RGBA16` on a deep batch; `pixels` are its bytes) composited on the device over each of `backgrounds`
    /// (samples at the side's depth) into reference slots `first_ref ..`: the pixel is read once.
    pub fn set_reference_over(&mut self, first_ref: u32, pixels: &[u8], format: i32, backgrounds: &[[u16; 3]]) -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_reference_over(self.handle, first_ref, pixels.as_ptr().cast(), pixels.len(), format,
                                             backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_over`: the same into test slots `first_pair ..`, pair `first_pair + k` bound to `ref_indices[k]`.
    pub fn set_test_over(&mut self, first_pair: u32, ref_indices: &[u32], pixels: &[u8], format: i32, backgrounds: &[[u16; 3]])
                         -> Result<(), HipError> {
        if ref_indices.len() != backgrounds.len() {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "one reference index per background".into() });
        }
        let rc = unsafe {
            sys::ce_batch_set_test_over(self.handle, first_pair, ref_indices.as_ptr(), pixels.as_ptr().cast(), pixels.len(), format,
                                        backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_cicp_over`: one straight-alpha RGBA image of tagged code values (`format`:
    /// `sys::CE_PIXEL_RGBA8` / `RGBA16`; `pixels` are its bytes) turned into linear light and blended there over each of
    /// `backgrounds` (linear light, sRGB primaries) into reference slots `first_ref ..` of a linear batch.
    pub fn set_reference_cicp_over(&mut self, first_ref: u32, pixels: &[u8], format: i32, colour: &sys::ce_colour, backgrounds: &[[f32; 3]])
                                   -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_reference_cicp_over(self.handle, first_ref, pixels.as_ptr().cast(), pixels.len(), format, colour,
                                                  backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_cicp_over`: the same into test slots `first_pair ..`, pair `first_pair + k` bound to `ref_indices[k]`.
    pub fn set_test_cicp_over(&mut self, first_pair: u32, ref_indices: &[u32], pixels: &[u8], format: i32, colour: &sys::ce_colour,
                              backgrounds: &[[f32; 3]]) -> Result<(), HipError> {
        self.one_ref_per_background(ref_indices, backgrounds)?;
        let rc = unsafe {
            sys::ce_batch_set_test_cicp_over(self.handle, first_pair, ref_indices.as_ptr(), pixels.as_ptr().cast(), pixels.len(), format,
                                             colour, backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_hlg_over`: the same for BT.2100 HLG code values read by `hlg`.
    pub fn set_reference_hlg_over(&mut self, first_ref: u32, pixels: &[u8], format: i32, hlg: &sys::ce_hlg, backgrounds: &[[f32; 3]])
                                  -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_reference_hlg_over(self.handle, first_ref, pixels.as_ptr().cast(), pixels.len(), format, hlg,
                                                 backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_hlg_over`
    pub fn set_test_hlg_over(&mut self, first_pair: u32, ref_indices: &[u32], pixels: &[u8], format: i32, hlg: &sys::ce_hlg,
                             backgrounds: &[[f32; 3]]) -> Result<(), HipError> {
        self.one_ref_per_background(ref_indices, backgrounds)?;
        let rc = unsafe {
            sys::ce_batch_set_test_hlg_over(self.handle, first_pair, ref_indices.as_ptr(), pixels.as_ptr().cast(), pixels.len(), format, hlg,
                                            backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_icc_over`: the same for code values of `depth` bits read through either flavour of profile.
    pub fn set_reference_icc_over(&mut self, first_ref: u32, pixels: &[u8], format: i32, depth: u32, icc: &HipIccProfile<'_>,
                                  backgrounds: &[[f32; 3]]) -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_reference_icc_over(self.handle, first_ref, pixels.as_ptr().cast(), pixels.len(), format, depth, icc.handle,
                                                 backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_icc_over`
    pub fn set_test_icc_over(&mut self, first_pair: u32, ref_indices: &[u32], pixels: &[u8], format: i32, depth: u32, icc: &HipIccProfile<'_>,
                             backgrounds: &[[f32; 3]]) -> Result<(), HipError> {
        self.one_ref_per_background(ref_indices, backgrounds)?;
        let rc = unsafe {
            sys::ce_batch_set_test_icc_over(self.handle, first_pair, ref_indices.as_ptr(), pixels.as_ptr().cast(), pixels.len(), format, depth,
                                            icc.handle, backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_linear_over`: float RGBA in linear light (`sys::CE_PIXEL_RGBA_F32`), straight or premultiplied.
    pub fn set_reference_linear_over(&mut self, first_ref: u32, rgba: &[f32], premultiplied: bool, backgrounds: &[[f32; 3]])
                                     -> Result<(), HipError> {
        let len = rgba.len() * 4;
        let rc = unsafe {
            sys::ce_batch_set_reference_linear_over(self.handle, first_ref, rgba.as_ptr().cast(), len, sys::CE_PIXEL_RGBA_F32,
                                                    premultiplied as i32, backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, len)
    }

    /// `ce_batch_set_test_linear_over`
    pub fn set_test_linear_over(&mut self, first_pair: u32, ref_indices: &[u32], rgba: &[f32], premultiplied: bool, backgrounds: &[[f32; 3]])
                                -> Result<(), HipError> {
        self.one_ref_per_background(ref_indices, backgrounds)?;
        let len = rgba.len() * 4;
        let rc = unsafe {
            sys::ce_batch_set_test_linear_over(self.handle, first_pair, ref_indices.as_ptr(), rgba.as_ptr().cast(), len, sys::CE_PIXEL_RGBA_F32,
                                               premultiplied as i32, backgrounds.len() as u32, backgrounds.as_ptr().cast())
        };
        self.check(rc, len)
    }

    fn one_ref_per_background(&self, ref_indices: &[u32], backgrounds: &[[f32; 3]]) -> Result<(), HipError> {
        if ref_indices.len() != backgrounds.len() {
            return Err(HipError::MetricCalculation { metric: "hip".into(), reason: "one reference index per background".into() });
        }
        Ok(())
    }

    /// `ce_batch_set_reference_icc`: code values of `depth` bits (`format` and `pixels` as `hlg_to_linear`) read through a
    /// matrix/TRC profile into a reference slot of any batch: linear light in a linear batch, sRGB code values of the slot's
    /// depth otherwise.
    pub fn set_reference_icc(&mut self, ref_index: u32, pixels: &[u8], format: i32, depth: u32, icc: &HipIccProfile<'_>) -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_reference_icc(self.handle, ref_index, pixels.as_ptr().cast(), pixels.len(), format, depth, icc.handle)
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_icc`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_icc(&mut self, pair_index: u32, ref_index: u32, pixels: &[u8], format: i32, depth: u32, icc: &HipIccProfile<'_>)
                        -> Result<(), HipError> {
        let rc = unsafe {
            sys::ce_batch_set_test_icc(self.handle, pair_index, ref_index, pixels.as_ptr().cast(), pixels.len(), format, depth, icc.handle)
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_yuv`: a decoder's planes straight into a reference slot.
    pub fn set_reference_yuv(&mut self, ref_index: u32, image: &YuvPlanes<'_>) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_reference_yuv(self.handle, ref_index, &c) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_test_yuv`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_yuv(&mut self, pair_index: u32, ref_index: u32, image: &YuvPlanes<'_>) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_test_yuv(self.handle, pair_index, ref_index, &c) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_reference_yuv_cicp`: a decoder's planes read by `colour` into a reference slot of a LINEAR batch.
    pub fn set_reference_yuv_cicp(&mut self, ref_index: u32, image: &YuvPlanes<'_>, colour: &sys::ce_colour) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_reference_yuv_cicp(self.handle, ref_index, &c, colour) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_test_yuv_cicp`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_yuv_cicp(&mut self, pair_index: u32, ref_index: u32, image: &YuvPlanes<'_>, colour: &sys::ce_colour)
                             -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_test_yuv_cicp(self.handle, pair_index, ref_index, &c, colour) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_reference_yuv_icc`: a decoder's planes read through `icc` (either flavour of profile) into a reference slot
    /// of any batch, in one kernel: linear light in a linear batch, sRGB code values of the slot's depth otherwise.  `rgb_depth`
    /// (8, 10, 12 or 16, not under the planes' depth) is the integer RGB grid between the colour matrix and the profile.
    pub fn set_reference_yuv_icc(&mut self, ref_index: u32, image: &YuvPlanes<'_>, rgb_depth: u32, icc: &HipIccProfile<'_>) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_reference_yuv_icc(self.handle, ref_index, &c, rgb_depth, icc.handle) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_test_yuv_icc`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_yuv_icc(&mut self, pair_index: u32, ref_index: u32, image: &YuvPlanes<'_>, rgb_depth: u32, icc: &HipIccProfile<'_>)
                            -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_test_yuv_icc(self.handle, pair_index, ref_index, &c, rgb_depth, icc.handle) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_reference_hlg`: BT.2100 HLG code values (`format` and `pixels` as `hlg_to_linear`) into a reference slot
    /// of a LINEAR batch.
    pub fn set_reference_hlg(&mut self, ref_index: u32, pixels: &[u8], format: i32, hlg: &sys::ce_hlg) -> Result<(), HipError> {
        let rc = unsafe { sys::ce_batch_set_reference_hlg(self.handle, ref_index, pixels.as_ptr().cast(), pixels.len(), format, hlg) };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_hlg`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_hlg(&mut self, pair_index: u32, ref_index: u32, pixels: &[u8], format: i32, hlg: &sys::ce_hlg) -> Result<(), HipError> {
        let rc = unsafe { sys::ce_batch_set_test_hlg(self.handle, pair_index, ref_index, pixels.as_ptr().cast(), pixels.len(), format, hlg) };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_gainmap`: an SDR base image (`format` and `pixels` as `hlg_to_linear`) read by `colour`, with
    /// the gain map `map` applied on the device, into a reference slot of a LINEAR batch.
    pub fn set_reference_gainmap(&mut self, ref_index: u32, pixels: &[u8], format: i32, colour: &sys::ce_colour, map: &GainMap<'_>)
                                 -> Result<(), HipError> {
        let image = map.to_sys()?;
        let rc = unsafe {
            sys::ce_batch_set_reference_gainmap(self.handle, ref_index, pixels.as_ptr().cast(), pixels.len(), format, colour, &image, &map.metadata)
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_test_gainmap`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_gainmap(&mut self, pair_index: u32, ref_index: u32, pixels: &[u8], format: i32, colour: &sys::ce_colour, map: &GainMap<'_>)
                            -> Result<(), HipError> {
        let image = map.to_sys()?;
        let rc = unsafe {
            sys::ce_batch_set_test_gainmap(self.handle, pair_index, ref_index, pixels.as_ptr().cast(), pixels.len(), format, colour, &image,
                                           &map.metadata)
        };
        self.check(rc, pixels.len())
    }

    /// `ce_batch_set_reference_tensor`: images `0 .. count` of a strided tensor of the batch's shape into reference slots
    /// `first_ref ..`; a device tensor is read in place by one launch, behind what the context's stream holds at the call.
    ///
    /// # Safety
    /// `t.data` and its strides must describe memory of the kind `t.memory` names that holds every element of `count`
    /// images; a device tensor must stay alive and unchanged until the batch's next launch has been collected.
    pub unsafe fn set_reference_tensor(&mut self, first_ref: u32, count: u32, t: &sys::ce_tensor_image) -> Result<(), HipError> {
        let rc = sys::ce_batch_set_reference_tensor(self.handle, first_ref, count, t);
        self.check(rc, 0)
    }

    /// `ce_batch_set_test_tensor`: the same into test slots `first_pair ..`, pair `first_pair + n` bound to reference
    /// `ref_indices[n]`; the tensor holds `ref_indices.len()` images.
    ///
    /// # Safety
    /// As `set_reference_tensor`.
    pub unsafe fn set_test_tensor(&mut self, first_pair: u32, ref_indices: &[u32], t: &sys::ce_tensor_image) -> Result<(), HipError> {
        let rc = sys::ce_batch_set_test_tensor(self.handle, first_pair, ref_indices.as_ptr(), ref_indices.len() as u32, t);
        self.check(rc, 0)
    }

    /// `ce_batch_set_reference_yuv_hlg`: a decoder's planes in HLG into a reference slot of a LINEAR batch.
    pub fn set_reference_yuv_hlg(&mut self, ref_index: u32, image: &YuvPlanes<'_>, hlg: &sys::ce_hlg) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_reference_yuv_hlg(self.handle, ref_index, &c, hlg) };
        self.check(rc, 0)
    }

    /// `ce_batch_set_test_yuv_hlg`: the same for the test image of pair `pair_index`, bound to reference `ref_index`.
    pub fn set_test_yuv_hlg(&mut self, pair_index: u32, ref_index: u32, image: &YuvPlanes<'_>, hlg: &sys::ce_hlg) -> Result<(), HipError> {
        let c = image.to_sys(self.width, self.height)?;
        let rc = unsafe { sys::ce_batch_set_test_yuv_hlg(self.handle, pair_index, ref_index, &c, hlg) };
        self.check(rc, 0)
    }

    /// `ce_batch_hdr_fidelity`: PQ-PSNR and BT.2124 Delta E ITP of pairs `[0, n_pairs)` of a LINEAR batch; returns once the
    /// scores are on the host.
    pub fn hdr_fidelity(&mut self, n_pairs: u32, depth: u32, white_nits: f32) -> Result<Vec<sys::ce_hdr_scores>, HipError> {
        let mut out = vec![sys::ce_hdr_scores::default(); n_pairs as usize];
        let rc = unsafe { sys::ce_batch_hdr_fidelity(self.handle, n_pairs, depth, white_nits, out.as_mut_ptr()) };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_msssim`: SSIM (`levels` 1) and MS-SSIM (5) of pairs `[0, n_pairs)` of an RGB8 or equal-depth deep batch on the
    /// encoded sample values; returns once the scores are on the host.
    pub fn ms_ssim(&mut self, n_pairs: u32, levels: u32) -> Result<Vec<sys::ce_msssim_scores>, HipError> {
        let mut out = vec![sys::ce_msssim_scores::default(); n_pairs as usize];
        let rc = unsafe { sys::ce_batch_msssim(self.handle, n_pairs, levels, out.as_mut_ptr()) };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_ciede2000`: CIEDE2000 of pairs `[0, n_pairs)` of an RGB8 or deep batch read as sRGB; `thresholds_q20` (at most
    /// eight, in units of 2^-20) are what `n_above` counts the pixels above; returns once the scores are on the host.
    pub fn ciede2000(&mut self, n_pairs: u32, thresholds_q20: &[u32]) -> Result<Vec<sys::ce_ciede2000_scores>, HipError> {
        let mut out = vec![sys::ce_ciede2000_scores::default(); n_pairs as usize];
        let rc = unsafe {
            sys::ce_batch_ciede2000(self.handle, n_pairs, thresholds_q20.as_ptr(), thresholds_q20.len() as u32, out.as_mut_ptr())
        };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_ciede2000_map`: where pairs `[first, first + count)` of an RGB8 or deep batch read as sRGB differ - the per-pixel
    /// map of `what` (`sys::CE_CIEDE2000_MAP_DE`, `_DL`, `_DC` or `_DH`) at `block` 1 or its block x block cell maxima when
    /// `want_map`, and how many pixels of each pair exceed each of up to `sys::CE_CIEDE2000_MAX_THRESHOLDS` thresholds; one of the
    /// two must be asked for.
    pub fn ciede2000_map(&mut self, first: u32, count: u32, what: u32, block: u32, want_map: bool, thresholds_q20: &[u32])
                         -> Result<Ciede2000Maps, HipError> {
        let mut out = Ciede2000Maps::sized(count, self.width, self.height, block, want_map, thresholds_q20.len());
        let rc = unsafe {
            sys::ce_batch_ciede2000_map(self.handle, first, count, what, block, out.map_ptr(), out.map.len(),
                                        slice_or_null(thresholds_q20), thresholds_q20.len() as u32, out.over_ptr())
        };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_msssim_map`: where pairs `[first, first + count)` of an RGB8 or equal-depth deep batch differ at `level` of the
    /// SSIM (`levels` 1) or MS-SSIM (5) pyramid - the per-position map of `what` (`sys::CE_MSSSIM_MAP_SSIM` or
    /// `sys::CE_MSSSIM_MAP_CS`) at `block` 1 or its block x block cell maxima when `want_map`, and how many positions of each pair
    /// and channel exceed each of up to `sys::CE_MSSSIM_MAP_MAX_THRESHOLDS` thresholds; one of the two must be asked for.
    pub fn ms_ssim_map(&mut self, first: u32, count: u32, levels: u32, level: u32, what: u32, block: u32, want_map: bool,
                       thresholds_q32: &[u32]) -> Result<MsSsimMaps, HipError> {
        let mut out = MsSsimMaps::sized(count, self.width, self.height, levels, level, block, want_map, thresholds_q32.len());
        let rc = unsafe {
            sys::ce_batch_msssim_map(self.handle, first, count, levels, level, what, block, out.map_ptr(), out.map.len(),
                                     slice_or_null(thresholds_q32), thresholds_q32.len() as u32, out.over_ptr())
        };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_delta_e_itp_map`: where pairs `[first, first + count)` of a LINEAR batch differ - the per-pixel Delta E ITP map
    /// (`block` 1) or its block x block cell maxima when `want_map`, and how many pixels of each pair exceed each of up to
    /// `sys::CE_DELTA_E_ITP_MAX_THRESHOLDS` thresholds; one of the two must be asked for.
    pub fn delta_e_itp_map(&mut self, first: u32, count: u32, depth: u32, white_nits: f32, block: u32, want_map: bool,
                           thresholds_q20: &[u32]) -> Result<DeltaEItpMaps, HipError> {
        let mut out = DeltaEItpMaps::sized(count, self.width, self.height, block, want_map, thresholds_q20.len());
        let rc = unsafe {
            sys::ce_batch_delta_e_itp_map(self.handle, first, count, depth, white_nits, block, out.map_ptr(), out.map.len(),
                                          slice_or_null(thresholds_q20), thresholds_q20.len() as u32, out.over_ptr())
        };
        self.check(rc, 0)?;
        Ok(out)
    }

    /// `ce_batch_resample`: references (`tests`: test images) `[first, first + count)` into the same indices of `dst`.
    pub fn resample_into(&mut self, dst: &mut HipBatch<'_>, tests: bool, first: u32, count: u32, filter: ResampleFilter)
                         -> Result<(), HipError> {
        let which = if tests { sys::CE_BATCH_TESTS } else { sys::CE_BATCH_REFERENCES };
        let rc = unsafe { sys::ce_batch_resample(self.handle, dst.handle, which, first, count, filter as i32) };
        self.check(rc, 0)
    }

    /// `ce_batch_resample_pairs`: both slabs and the pair bindings; `dst.run(n_pairs, ..)` follows directly.
    pub fn resample_pairs_into(&mut self, dst: &mut HipBatch<'_>, n_refs: u32, n_pairs: u32, filter: ResampleFilter)
                               -> Result<(), HipError> {
        let rc = unsafe { sys::ce_batch_resample_pairs(self.handle, dst.handle, n_refs, n_pairs, filter as i32) };
        self.check(rc, 0)
    }

    /// `ce_batch_run` over pairs `[0, n_pairs)`.
    pub fn run(&mut self, n_pairs: u32, m: Metrics) -> Result<Vec<Scores>, HipError> {
        let mut out = vec![sys::ce_scores::default(); n_pairs as usize];
        let rc = unsafe {
            sys::ce_batch_run(self.handle, n_pairs, m.mask(), m.flags(), sys::CE_DEFAULT_INTENSITY_TARGET, out.as_mut_ptr())
        };
        self.check(rc, 0)?;
        Ok(out.into_iter().map(Into::into).collect())
    }
}

impl Drop for HipBatch<'_> {
    fn drop(&mut self) {
        unsafe { sys::ce_batch_destroy(self.handle) }
    }
}
