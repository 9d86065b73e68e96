// codec_eval.hpp — C++17 host-side mirror of the reference's interface for the metric hot path, written
// on top of the C ABI (include/ce_metrics.h).  The reference is a Rust crate and no Rust toolchain exists
// in the build image, so this header plays the part the Rust `hip` feature would play:
// same names, argument meaning and error behaviour as
//   src/metrics/mod.rs        MetricConfig, MetricResult, PerceptionLevel, calculate_psnr
//   src/metrics/{ssimulacra2,dssim,butteraugli,xyb}.rs   the leaf functions
//   src/eval/session.rs       ImageData, EncodeRequest, EvalConfig, EvalSession::evaluate_image
//   src/eval/helpers.rs       evaluate_single, assert_quality, assert_perception_level
//   src/eval/report.rs        CodecResult, ImageReport
// The one deliberate difference: evaluate_image runs every encode/decode callback first and then scores
// the whole (codec x quality) grid with ONE ce_eval_batch call (the reference scores inside the double
// loop, session.rs:375-410); results are emitted in the reference's loop order.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ce_metrics.h"

namespace codec_eval {

// ---- src/error.rs:31-75 (the variants this path can raise) -----------------------------------------
struct Error : std::runtime_error {
    enum class Kind { DimensionMismatch, MetricCalculation, QualityBelowThreshold, Codec };
    Kind kind;
    Error(Kind k, const std::string &what) : std::runtime_error(what), kind(k) {}
};

// ---- src/metrics/mod.rs:46-136 ------------------------------------------------------------------------
struct MetricConfig {
    bool dssim = false, ssimulacra2 = false, butteraugli = false, psnr = false, xyb_roundtrip = false;
    static MetricConfig all() { return {true, true, true, true, false}; }
    static MetricConfig fast() { return {false, false, false, true, false}; }
    static MetricConfig perceptual() { return {true, true, true, false, false}; }
    static MetricConfig perceptual_xyb() { return {true, true, true, false, true}; }
    static MetricConfig ssimulacra2_only() { return {false, true, false, false, false}; }
    MetricConfig with_xyb_roundtrip() const { MetricConfig c = *this; c.xyb_roundtrip = true; return c; }
    uint32_t mask() const
    {
        return (dssim ? (uint32_t)CE_METRIC_DSSIM : 0u) | (ssimulacra2 ? (uint32_t)CE_METRIC_SSIMULACRA2 : 0u) |
               (butteraugli ? (uint32_t)CE_METRIC_BUTTERAUGLI : 0u) | (psnr ? (uint32_t)CE_METRIC_PSNR : 0u);
    }
    uint32_t flags() const { return xyb_roundtrip ? (uint32_t)CE_FLAG_XYB_ROUNDTRIP : 0u; }
};

// ---- src/metrics/mod.rs:172-284 -----------------------------------------------------------------------
enum class PerceptionLevel : uint8_t { Imperceptible, Marginal, Subtle, Noticeable, Degraded };

inline PerceptionLevel perception_from_dssim(double d)
{
    return d < 0.0003 ? PerceptionLevel::Imperceptible : d < 0.0007 ? PerceptionLevel::Marginal
         : d < 0.0015 ? PerceptionLevel::Subtle : d < 0.003 ? PerceptionLevel::Noticeable : PerceptionLevel::Degraded;
}
inline PerceptionLevel perception_from_ssimulacra2(double s)
{
    return s > 90.0 ? PerceptionLevel::Imperceptible : s > 80.0 ? PerceptionLevel::Marginal
         : s > 70.0 ? PerceptionLevel::Subtle : s > 50.0 ? PerceptionLevel::Noticeable : PerceptionLevel::Degraded;
}
inline PerceptionLevel perception_from_butteraugli(double b)
{
    return b < 1.0 ? PerceptionLevel::Imperceptible : b < 2.0 ? PerceptionLevel::Marginal
         : b < 3.0 ? PerceptionLevel::Subtle : b < 5.0 ? PerceptionLevel::Noticeable : PerceptionLevel::Degraded;
}
inline const char *perception_code(PerceptionLevel l)
{
    static const char *const c[] = {"IMP", "MAR", "SUB", "NOT", "DEG"};
    return c[(int)l];
}

// ---- src/metrics/mod.rs:138-169 -----------------------------------------------------------------------
struct MetricResult {
    std::optional<double> dssim, ssimulacra2, butteraugli, psnr;
    std::optional<PerceptionLevel> perception_level() const
    {
        return dssim ? std::optional<PerceptionLevel>(perception_from_dssim(*dssim)) : std::nullopt;
    }
    static MetricResult from_c(const ce_scores &s)
    {
        MetricResult r;
        if (s.valid & CE_METRIC_DSSIM) r.dssim = s.dssim;
        if (s.valid & CE_METRIC_SSIMULACRA2) r.ssimulacra2 = s.ssimulacra2;
        if (s.valid & CE_METRIC_BUTTERAUGLI) r.butteraugli = s.butteraugli;
        if (s.valid & CE_METRIC_PSNR) r.psnr = s.psnr;
        return r;
    }
};

// ---- the device context (GpuSsim2::new / Drop, crates/codec-iter/src/gpu.rs:40-80,118-133) ------------
class HipBackend {
public:
    explicit HipBackend(int device = 0)
    {
        if (ce_ctx_create(device, &ctx_) != CE_OK)
            throw Error(Error::Kind::MetricCalculation, std::string("HIP init failed: ") + ce_last_error(nullptr));
    }
    ~HipBackend() { ce_ctx_destroy(ctx_); }
    HipBackend(const HipBackend &) = delete;
    HipBackend &operator=(const HipBackend &) = delete;
    ce_ctx *ctx() const { return ctx_; }
    std::string last_error() const { return ce_last_error(ctx_); }
    static int device_count() { return ce_device_count(); }

private:
    ce_ctx *ctx_ = nullptr;
};

namespace detail {
inline void check(const HipBackend &be, int rc, const char *metric, size_t w, size_t h, size_t test_len)
{
    if (rc == CE_OK) return;
    if (rc == CE_ERR_DIM_MISMATCH)  // ssimulacra2.rs:65-70
        throw Error(Error::Kind::DimensionMismatch, "Dimension mismatch: expected (" + std::to_string(w) + ", " + std::to_string(h) +
                                                        "), got (" + std::to_string(h ? test_len / 3 / h : 0) + ", " + std::to_string(h) + ")");
    throw Error(Error::Kind::MetricCalculation, std::string("Metric calculation failed: ") + metric + ": " + be.last_error());
}
}  // namespace detail

namespace metrics {
using Bytes = std::vector<uint8_t>;

// calculate_psnr, src/metrics/mod.rs:312-331.  The reference asserts on bad lengths; so does this.
inline double calculate_psnr(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width, size_t height)
{
    if (reference.size() != test.size()) throw std::logic_error("assertion failed: reference.len() == test.len()");
    if (reference.size() != width * height * 3) throw std::logic_error("assertion failed: reference.len() == width * height * 3");
    double out = 0;
    detail::check(be, ce_calculate_psnr(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height, &out),
                  "PSNR", width, height, test.size());
    return out;
}
// calculate_ssimulacra2, src/metrics/ssimulacra2.rs:59-100
inline double calculate_ssimulacra2(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width, size_t height)
{
    double out = 0;
    detail::check(be, ce_calculate_ssimulacra2(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height, &out),
                  "SSIMULACRA2", width, height, test.size());
    return out;
}
// rgb8_to_dssim_image x2 + calculate_dssim, src/metrics/dssim.rs:102-114,40-71 (session.rs:467-476 composes them)
inline double calculate_dssim(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width, size_t height)
{
    double out = 0;
    detail::check(be, ce_calculate_dssim(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height, &out),
                  "DSSIM", width, height, test.size());
    return out;
}
// calculate_butteraugli / _with_intensity, src/metrics/butteraugli.rs:45-136
inline double calculate_butteraugli_with_intensity(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width,
                                                   size_t height, float intensity_target)
{
    double out = 0;
    detail::check(be, ce_calculate_butteraugli(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height,
                                               intensity_target, &out),
                  "Butteraugli", width, height, test.size());
    return out;
}
inline double calculate_butteraugli(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width, size_t height)
{
    return calculate_butteraugli_with_intensity(be, reference, test, width, height, CE_DEFAULT_INTENSITY_TARGET);
}
// ButteraugliResult{score, diffmap}, src/metrics/prelude.rs:64-65: diffmap is row-major width * height, its maximum the score
struct ButteraugliResult {
    double score;
    std::vector<float> diffmap;
};
inline ButteraugliResult calculate_butteraugli_with_diffmap(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width,
                                                            size_t height, float intensity_target = CE_DEFAULT_INTENSITY_TARGET)
{
    ButteraugliResult r{0.0, std::vector<float>(width * height)};
    detail::check(be, ce_calculate_butteraugli_diffmap(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height,
                                                       intensity_target, &r.score, r.diffmap.data()),
                  "Butteraugli", width, height, test.size());
    return r;
}
// dssim-core's SsimMap (re-exported at src/metrics/prelude.rs:45): one scale's per-pixel SSIM image, row-major
// width * height, and that scale's pooled score
struct SsimMap {
    size_t width, height;
    std::vector<float> map;
    double ssim;
};
// calculate_dssim with the maps kept, the shape of Dssim::compare ((Val, Vec<SsimMap>), dropped at src/metrics/dssim.rs:68):
// the score and one SsimMap per scale, level 0 at full resolution
inline std::pair<double, std::vector<SsimMap>> calculate_dssim_with_ssim_maps(const HipBackend &be, const Bytes &reference,
                                                                              const Bytes &test, size_t width, size_t height)
{
    uint32_t n = 0, lw[CE_DSSIM_MAX_LEVELS] = {}, lh[CE_DSSIM_MAX_LEVELS] = {};
    if (width > 0 && height > 0 && width <= UINT32_MAX && height <= UINT32_MAX)
        ce_dssim_levels((uint32_t)width, (uint32_t)height, &n, lw, lh);
    size_t total = 0;
    for (uint32_t l = 0; l < n; l++) total += (size_t)lw[l] * lh[l];
    std::vector<float> maps(total);
    double score = 0.0, ssim[CE_DSSIM_MAX_LEVELS];
    detail::check(be, ce_calculate_dssim_ssim_maps(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height,
                                                   &score, ssim, maps.data(), maps.size()),
                  "DSSIM", width, height, test.size());
    std::vector<SsimMap> out;
    size_t off = 0;
    for (uint32_t l = 0; l < n; l++) {
        const size_t m = (size_t)lw[l] * lh[l];
        out.push_back(SsimMap{lw[l], lh[l], std::vector<float>(maps.begin() + off, maps.begin() + off + m), ssim[l]});
        off += m;
    }
    return {score, std::move(out)};
}
// One scale of SSIMULACRA2's per-pixel error terms (ssim_map / edge_diff_map of the lineage behind src/metrics/ssimulacra2.rs:96):
// maps is [channel 3][kind 3][height][width], kinds in enum ce_ssim2_map order (SSIM, artifact, detail lost)
struct Ssim2Maps {
    size_t width, height;
    std::vector<float> maps;
};
struct Ssim2WithMaps {
    double score;
    double features[CE_SSIM2_MAX_SCALES * 18];  // [scale][channel][6]: the means and 4-norms the score weighs, NaN past the scales
    std::vector<Ssim2Maps> scales;              // scale 0 at full resolution
};
// calculate_ssimulacra2 (src/metrics/ssimulacra2.rs:59) with everything the score pools kept
inline Ssim2WithMaps calculate_ssimulacra2_with_maps(const HipBackend &be, const Bytes &reference, const Bytes &test, size_t width,
                                                     size_t height)
{
    uint32_t n = 0, sw[CE_SSIM2_MAX_SCALES] = {}, sh[CE_SSIM2_MAX_SCALES] = {};
    if (width > 0 && height > 0 && width <= UINT32_MAX && height <= UINT32_MAX)
        ce_ssimulacra2_scales((uint32_t)width, (uint32_t)height, &n, sw, sh);
    size_t total = 0;
    for (uint32_t s = 0; s < n; s++) total += 9 * (size_t)sw[s] * sh[s];
    std::vector<float> maps(total);
    Ssim2WithMaps r{};
    detail::check(be, ce_calculate_ssimulacra2_maps(be.ctx(), reference.data(), reference.size(), test.data(), test.size(), width, height,
                                                    &r.score, r.features, maps.data(), maps.size()),
                  "SSIMULACRA2", width, height, test.size());
    size_t off = 0;
    for (uint32_t s = 0; s < n; s++) {
        const size_t m = 9 * (size_t)sw[s] * sh[s];
        r.scales.push_back(Ssim2Maps{sw[s], sh[s], std::vector<float>(maps.begin() + off, maps.begin() + off + m)});
        off += m;
    }
    return r;
}
// xyb_roundtrip, src/metrics/xyb.rs:225-253 (asserts on the length, :227)
inline Bytes xyb_roundtrip(const HipBackend &be, const Bytes &rgb, size_t width, size_t height)
{
    if (rgb.size() != width * height * 3) throw std::logic_error("Buffer size mismatch");
    Bytes out(rgb.size());
    detail::check(be, ce_xyb_roundtrip(be.ctx(), rgb.data(), rgb.size(), width, height, out.data()), "XYB", width, height, rgb.size());
    return out;
}
// rgb8_to_dssim_image, src/metrics/dssim.rs:102-114: RGBA f32, linear light, a = 1.0
inline std::vector<float> rgb8_to_dssim_image(const HipBackend &be, const Bytes &rgb, size_t width, size_t height)
{
    std::vector<float> out(width * height * 4);
    detail::check(be, ce_rgb8_to_dssim_image(be.ctx(), rgb.data(), rgb.size(), width, height, out.data()), "DSSIM", width, height, rgb.size());
    return out;
}
// compute_heuristics (crates/codec-compare/src/image_heuristics.rs:76-305) of packed RGB8; under 3 x 3 is an error (the
// reference panics there)
inline ce_image_heuristics compute_heuristics(const HipBackend &be, const Bytes &rgb, size_t width, size_t height)
{
    ce_image_heuristics h{};
    detail::check(be, ce_image_heuristics_rgb8(be.ctx(), rgb.data(), rgb.size(), width, height, &h), "image heuristics", width, height,
                  rgb.size());
    return h;
}
}  // namespace metrics

// ---- src/viewing.rs: viewing conditions ------------------------------------------------------------------------------
// ViewingCondition, SimulationMode, SimulationParams, REFERENCE_PPD and the presets, item for item (every formula f64,
// std::round = f64::round: half away from zero).  The reference stops at the parameters; displayed_size() and
// metrics::resample_rgb8 / ce_batch_resample go on to the image a viewer sees.
namespace viewing {

constexpr double REFERENCE_PPD = 40.0;  // viewing.rs:337

enum class SimulationMode { Accurate, DownsampleOnly };  // viewing.rs:33-53

namespace detail {
inline uint32_t round_u32(double x)  // `x.round() as u32`: the cast saturates
{
    const double r = std::round(x);
    if (!(r > 0.0)) return 0;
    return r >= 4294967295.0 ? 4294967295u : (uint32_t)r;
}
}  // namespace detail

struct SimulationParams {  // viewing.rs:308-331
    double scale_factor = 1.0;
    uint32_t target_width = 0, target_height = 0;
    double adjusted_ppd = REFERENCE_PPD;
    bool requires_upscale = false, requires_downscale = false;

    bool requires_scaling() const { return requires_upscale || requires_downscale; }
    double downscale_only_factor() const { return std::min(scale_factor, 1.0); }
    double threshold_multiplier() const { return adjusted_ppd / REFERENCE_PPD; }
    double adjust_dssim_threshold(double base) const { return base * threshold_multiplier(); }
    double adjust_butteraugli_threshold(double base) const { return base * threshold_multiplier(); }
    double adjust_ssimulacra2_threshold(double base) const  // viewing.rs:431-445
    {
        const double m = threshold_multiplier();
        const double v = m >= 1.0 ? base - (100.0 - base) * (1.0 - 1.0 / m) : base + (100.0 - base) * (1.0 / m - 1.0);
        return std::min(std::max(v, 0.0), 100.0);
    }
    bool dssim_acceptable(double dssim, double base) const { return dssim < adjust_dssim_threshold(base); }
    bool butteraugli_acceptable(double b, double base) const { return b < adjust_butteraugli_threshold(base); }
    bool ssimulacra2_acceptable(double s, double base) const { return s > adjust_ssimulacra2_threshold(base); }
    // Not in the reference: the device pixels a width x height image occupies, round(n / scale_factor) per side and at
    // least 1 - the size it is resampled to (target_width multiplies where a browser divides; the reference's tests pin it)
    std::pair<uint32_t, uint32_t> displayed_size(uint32_t width, uint32_t height) const
    {
        if (scale_factor == 1.0) return {width, height};
        return {std::max(1u, detail::round_u32((double)width / scale_factor)), std::max(1u, detail::round_u32((double)height / scale_factor))};
    }
};

struct ViewingCondition {  // viewing.rs:74-104
    double acuity_ppd = 40.0;  // Default = desktop(), viewing.rs:471-475
    std::optional<double> browser_dppx, image_intrinsic_dppx, ppd;

    static ViewingCondition make(double acuity_ppd) { return {acuity_ppd, std::nullopt, std::nullopt, std::nullopt}; }  // ::new
    static ViewingCondition desktop() { return make(40.0); }
    static ViewingCondition laptop() { return make(60.0); }
    static ViewingCondition smartphone() { return make(90.0); }
    ViewingCondition with_browser_dppx(double dppx) const
    {
        ViewingCondition v = *this;
        v.browser_dppx = dppx;
        return v;
    }
    ViewingCondition with_image_intrinsic_dppx(double dppx) const
    {
        ViewingCondition v = *this;
        v.image_intrinsic_dppx = dppx;
        return v;
    }
    ViewingCondition with_ppd_override(double p) const
    {
        ViewingCondition v = *this;
        v.ppd = p;
        return v;
    }
    double srcset_ratio() const { return image_intrinsic_dppx.value_or(1.0) / browser_dppx.value_or(1.0); }
    double effective_ppd() const { return ppd ? *ppd : acuity_ppd * srcset_ratio(); }
    SimulationParams simulation_params(uint32_t w, uint32_t h, SimulationMode mode) const  // viewing.rs:244-301
    {
        const double ratio = srcset_ratio();
        if (mode == SimulationMode::Accurate || ratio >= 1.0)
            return {ratio, detail::round_u32((double)w * ratio), detail::round_u32((double)h * ratio), effective_ppd(),
                    mode == SimulationMode::Accurate && ratio < 1.0, ratio > 1.0};
        return {1.0, w, h, acuity_ppd * ratio, false, false};
    }
    bool operator==(const ViewingCondition &o) const
    {
        return acuity_ppd == o.acuity_ppd && browser_dppx == o.browser_dppx && image_intrinsic_dppx == o.image_intrinsic_dppx && ppd == o.ppd;
    }
};

namespace presets {  // viewing.rs:495-656
inline ViewingCondition of(double acuity, double browser, double intrinsic)
{
    return ViewingCondition::make(acuity).with_browser_dppx(browser).with_image_intrinsic_dppx(intrinsic);
}
inline ViewingCondition native_desktop() { return of(40.0, 1.0, 1.0); }
inline ViewingCondition native_laptop() { return of(70.0, 2.0, 2.0); }
inline ViewingCondition native_phone() { return of(95.0, 3.0, 3.0); }
inline ViewingCondition srcset_1x_on_phone() { return of(95.0, 3.0, 1.0); }
inline ViewingCondition srcset_1x_on_laptop() { return of(70.0, 2.0, 1.0); }
inline ViewingCondition srcset_2x_on_phone() { return of(95.0, 3.0, 2.0); }
inline ViewingCondition srcset_2x_on_desktop() { return of(40.0, 1.0, 2.0); }
inline ViewingCondition srcset_2x_on_laptop_1_5x() { return of(70.0, 1.5, 2.0); }
inline ViewingCondition srcset_3x_on_phone() { return native_phone(); }
inline std::vector<ViewingCondition> all()  // most demanding first
{
    return {srcset_1x_on_phone(), srcset_1x_on_laptop(), native_desktop(),           srcset_2x_on_phone(),
            native_laptop(),      srcset_2x_on_desktop(), srcset_2x_on_laptop_1_5x(), native_phone()};
}
inline std::vector<ViewingCondition> key() { return {native_desktop(), native_laptop(), native_phone()}; }
inline ViewingCondition baseline() { return native_laptop(); }
inline ViewingCondition demanding() { return native_desktop(); }
}  // namespace presets
}  // namespace viewing

namespace metrics {
// One packed RGB8 image at another size (ce_resample_rgb8): what SimulationParams (viewing.rs:308-331) describes
inline Bytes resample_rgb8(const HipBackend &be, const Bytes &rgb, uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height,
                           int filter = CE_RESAMPLE_LANCZOS3)
{
    Bytes out((size_t)out_width * out_height * 3);
    detail::check(be, ce_resample_rgb8(be.ctx(), rgb.data(), rgb.size(), width, height, out_width, out_height, filter, out.data(), out.size()),
                  "resample", width, height, rgb.size());
    return out;
}

// One packed float RGB image in linear light at another size (ce_resample_linear): the convolution
// of Pillow's Image.resize on mode "F" images, bit for bit, clamped to +-CE_LINEAR_MAX
inline std::vector<float> resample_linear(const HipBackend &be, const std::vector<float> &rgb, uint32_t width, uint32_t height, uint32_t out_width,
                                          uint32_t out_height, int filter = CE_RESAMPLE_LANCZOS3)
{
    std::vector<float> out((size_t)out_width * out_height * 3);
    detail::check(be, ce_resample_linear(be.ctx(), rgb.data(), rgb.size() * 4, width, height, out_width, out_height, filter, out.data(), out.size() * 4),
                  "resample", width, height, rgb.size());
    return out;
}

// ---- planar Y'CbCr ingest: a decoder's planes, upsampled and converted on the device -------------
// The struct is the ABI's; yuv_image() fills the common case (8-bit 4:2:0 planar, BT.601 full range, triangle upsampling:
// what a JPEG decoder in raw mode hands over) and the caller changes what differs.
using YuvImage = ce_yuv_image;
inline YuvImage yuv_image(const void *y, size_t y_pitch, const void *cb, size_t cb_pitch, const void *cr, size_t cr_pitch,
                          int memory = CE_MEM_HOST)
{
    YuvImage img{};
    img.plane[0] = y, img.plane[1] = cb, img.plane[2] = cr;
    img.pitch[0] = y_pitch, img.pitch[1] = cb_pitch, img.pitch[2] = cr_pitch;
    img.subsampling = CE_YUV_420, img.layout = CE_YUV_PLANAR, img.matrix = CE_YUV_BT601, img.range = CE_YUV_FULL;
    img.upsample = CE_CHROMA_TRIANGLE, img.depth = 8, img.msb_aligned = 0, img.memory = memory, img.lut = nullptr;
    return img;
}
inline Bytes yuv_to_rgb8(const HipBackend &be, const YuvImage &image, uint32_t width, uint32_t height)
{
    Bytes out((size_t)width * height * 3);
    detail::check(be, ce_yuv_to_rgb8(be.ctx(), &image, width, height, out.data(), out.size()), "yuv", width, height, out.size());
    return out;
}
inline std::vector<uint16_t> yuv_to_rgb16(const HipBackend &be, const YuvImage &image, uint32_t width, uint32_t height, uint32_t depth_out)
{
    std::vector<uint16_t> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_to_rgb16(be.ctx(), &image, width, height, depth_out, out.data(), out.size()), "yuv", width, height, out.size());
    return out;
}
// ---- CICP ingest (include/ce_metrics.h: ce_cicp_to_linear) ---------------------------------------
// H.273 code points a decoder reports; presets for the common three
using ColourDescription = ce_colour;
inline ColourDescription colour_srgb(uint32_t depth = 8) { return ColourDescription{1, 13, depth, 0.0f}; }
inline ColourDescription colour_display_p3(uint32_t depth = 8) { return ColourDescription{12, 13, depth, 0.0f}; }
inline ColourDescription colour_bt2020_pq(uint32_t depth = 10, float white_nits = 203.0f) { return ColourDescription{9, 16, depth, white_nits}; }
// One image of integer RGB(A) code values (format: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16; len in bytes) read by `colour`
// -> packed float RGB, linear light with BT.709 / sRGB primaries, on the device
inline std::vector<float> cicp_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, const ColourDescription &colour,
                                         uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_cicp_to_linear(be.ctx(), pixels, len, format, &colour, width, height, out.data(), out.size()), "cicp", width, height, len);
    return out;
}
// straight into a slot of a linear batch (eval::batch_linear)
inline void batch_set_reference_cicp(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const void *pixels, size_t len, int format,
                                     const ColourDescription &colour)
{
    detail::check(be, ce_batch_set_reference_cicp(batch, ref_index, pixels, len, format, &colour), "cicp", 0, 0, 0);
}
inline void batch_set_test_cicp(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len,
                                int format, const ColourDescription &colour)
{
    detail::check(be, ce_batch_set_test_cicp(batch, pair_index, ref_index, pixels, len, format, &colour), "cicp", 0, 0, 0);
}
// ---- matrix/TRC ICC profiles applied on the device (include/ce_metrics.h: ce_icc_*) -------------------
// what the library's parser reads from a profile, without a device: kind CE_ICC_SUPPORTED for the profiles HipIccProfile takes
inline ce_icc_description icc_describe(const std::vector<uint8_t> &icc_profile)
{
    ce_icc_description d{};
    ce_icc_describe(icc_profile.data() ? icc_profile.data() : reinterpret_cast<const uint8_t *>(""), icc_profile.size(), &d);
    return d;
}
// what the parser of LUT-based profiles reads, without a device: kind CE_ICC_LUT_SUPPORTED for those the four-argument
// constructor of HipIccProfile takes
inline ce_icc_lut_description icc_lut_describe(const std::vector<uint8_t> &icc_profile, int intent = 0)
{
    ce_icc_lut_description d{};
    ce_icc_lut_describe(icc_profile.data() ? icc_profile.data() : reinterpret_cast<const uint8_t *>(""), icc_profile.size(), intent, &d);
    return d;
}
// A profile of three colorants and three tone curves on the device, parsed by the library itself (no Cms).  A LUT-based, Gray,
// CMYK or malformed profile throws with the reason; those keep HipColorTable's route.
class HipIccProfile {
public:
    HipIccProfile(const HipBackend &be, const std::vector<uint8_t> &icc_profile)
    {
        if (ce_icc_create(be.ctx(), icc_profile.data(), icc_profile.size(), &icc_) != CE_OK)
            throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: ICC: Failed to create ICC transform: " + be.last_error());
    }
    // a LUT-based profile (an A2B tag of type mAB, mft2 or mft1) evaluated from the profile itself: intent
    // 0, 1 or 2 chooses A2B0 / A2B1 / A2B2, interpolation is CE_ICC_CLUT_TRILINEAR or CE_ICC_CLUT_TETRAHEDRAL
    HipIccProfile(const HipBackend &be, const std::vector<uint8_t> &icc_profile, int intent, int interpolation)
    {
        if (ce_icc_lut_create(be.ctx(), icc_profile.data(), icc_profile.size(), intent, interpolation, &icc_) != CE_OK)
            throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: ICC: Failed to create ICC transform: " + be.last_error());
    }
    ~HipIccProfile() { ce_icc_destroy(icc_); }
    HipIccProfile(const HipIccProfile &) = delete;
    HipIccProfile &operator=(const HipIccProfile &) = delete;
    const ce_icc *get() const { return icc_; }

private:
    ce_icc *icc_ = nullptr;
};
// One image of integer RGB(A) code values of `depth` bits (format: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16; len in bytes) read
// through the profile -> packed float RGB, linear light with sRGB primaries; -> packed sRGB8; -> packed u16 sRGB of depth_out
inline std::vector<float> icc_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, uint32_t depth, const HipIccProfile &icc,
                                        uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_icc_to_linear(be.ctx(), pixels, len, format, depth, icc.get(), width, height, out.data(), out.size()), "icc", width, height, len);
    return out;
}
inline std::vector<uint8_t> icc_to_srgb8(const HipBackend &be, const void *pixels, size_t len, int format, uint32_t depth, const HipIccProfile &icc,
                                         uint32_t width, uint32_t height)
{
    std::vector<uint8_t> out((size_t)width * height * 3);
    detail::check(be, ce_icc_to_srgb8(be.ctx(), pixels, len, format, depth, icc.get(), width, height, out.data(), out.size()), "icc", width, height, len);
    return out;
}
inline std::vector<uint16_t> icc_to_srgb16(const HipBackend &be, const void *pixels, size_t len, int format, uint32_t depth, const HipIccProfile &icc,
                                           uint32_t width, uint32_t height, uint32_t depth_out)
{
    std::vector<uint16_t> out((size_t)width * height * 3);
    detail::check(be, ce_icc_to_srgb16(be.ctx(), pixels, len, format, depth, icc.get(), width, height, depth_out, out.data(), out.size()), "icc", width,
                  height, len);
    return out;
}
// straight into a slot of any batch: linear light in a linear batch, sRGB code values of the slot's depth otherwise
inline void batch_set_reference_icc(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const void *pixels, size_t len, int format,
                                    uint32_t depth, const HipIccProfile &icc)
{
    detail::check(be, ce_batch_set_reference_icc(batch, ref_index, pixels, len, format, depth, icc.get()), "icc", 0, 0, 0);
}
inline void batch_set_test_icc(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len,
                               int format, uint32_t depth, const HipIccProfile &icc)
{
    detail::check(be, ce_batch_set_test_icc(batch, pair_index, ref_index, pixels, len, format, depth, icc.get()), "icc", 0, 0, 0);
}
// ---- Y'CbCr planes with a colour description -> linear light in one kernel ---------------------------
// yuv_to_rgb16 at depth_out = colour.depth followed by cicp_to_linear, bit for bit; colour.depth >= image.depth
inline std::vector<float> yuv_to_linear(const HipBackend &be, const YuvImage &image, const ColourDescription &colour, uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_to_linear(be.ctx(), &image, &colour, width, height, out.data(), out.size()), "yuv_cicp", width, height, out.size());
    return out;
}
// straight into a slot of a linear batch (eval::batch_linear), host or device planes
inline void batch_set_reference_yuv_cicp(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const YuvImage &image, const ColourDescription &colour)
{
    detail::check(be, ce_batch_set_reference_yuv_cicp(batch, ref_index, &image, &colour), "yuv_cicp", 0, 0, 0);
}
inline void batch_set_test_yuv_cicp(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const YuvImage &image,
                                    const ColourDescription &colour)
{
    detail::check(be, ce_batch_set_test_yuv_cicp(batch, pair_index, ref_index, &image, &colour), "yuv_cicp", 0, 0, 0);
}
// ---- Y'CbCr planes with an ICC profile, in one kernel (include/ce_metrics.h: ce_batch_set_*_yuv_icc) ----
// rgb_depth (8, 10, 12 or 16, not under the planes' depth): the integer RGB grid between the colour matrix and the profile
inline std::vector<float> yuv_icc_to_linear(const HipBackend &be, const YuvImage &image, uint32_t rgb_depth, const HipIccProfile &icc, uint32_t width,
                                            uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_icc_to_linear(be.ctx(), &image, rgb_depth, icc.get(), width, height, out.data(), out.size()), "yuv_icc", width, height, out.size());
    return out;
}
inline std::vector<uint8_t> yuv_icc_to_srgb8(const HipBackend &be, const YuvImage &image, uint32_t rgb_depth, const HipIccProfile &icc, uint32_t width,
                                             uint32_t height)
{
    std::vector<uint8_t> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_icc_to_srgb8(be.ctx(), &image, rgb_depth, icc.get(), width, height, out.data(), out.size()), "yuv_icc", width, height, out.size());
    return out;
}
inline std::vector<uint16_t> yuv_icc_to_srgb16(const HipBackend &be, const YuvImage &image, uint32_t rgb_depth, const HipIccProfile &icc, uint32_t width,
                                               uint32_t height, uint32_t depth_out)
{
    std::vector<uint16_t> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_icc_to_srgb16(be.ctx(), &image, rgb_depth, icc.get(), width, height, depth_out, out.data(), out.size()), "yuv_icc", width,
                  height, out.size());
    return out;
}
// straight into a slot of any batch, host or device planes: linear light in a linear batch, sRGB code values of the slot's depth otherwise
inline void batch_set_reference_yuv_icc(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const YuvImage &image, uint32_t rgb_depth,
                                        const HipIccProfile &icc)
{
    detail::check(be, ce_batch_set_reference_yuv_icc(batch, ref_index, &image, rgb_depth, icc.get()), "yuv_icc", 0, 0, 0);
}
inline void batch_set_test_yuv_icc(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const YuvImage &image,
                                   uint32_t rgb_depth, const HipIccProfile &icc)
{
    detail::check(be, ce_batch_set_test_yuv_icc(batch, pair_index, ref_index, &image, rgb_depth, icc.get()), "yuv_icc", 0, 0, 0);
}
// ---- BT.2100 HLG -> display light, linear, with sRGB primaries (include/ce_metrics.h: ce_hlg_to_linear) ----
// HLG carries the display it is shown on - peak luminance and system gamma (0: BT.2100's rule from the peak) - besides the
// primaries, the depth and the luminance that becomes 1.0
using HlgDescription = ce_hlg;
inline HlgDescription hlg_bt2100(uint32_t depth = 10, float peak_nits = 1000.0f, float white_nits = 203.0f)
{
    return HlgDescription{9, depth, peak_nits, 0.0f, white_nits};
}
// One image of integer RGB(A) HLG code values (format: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16; len in bytes) -> packed float RGB
inline std::vector<float> hlg_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, const HlgDescription &hlg,
                                        uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_hlg_to_linear(be.ctx(), pixels, len, format, &hlg, width, height, out.data(), out.size()), "hlg", width, height, len);
    return out;
}
// straight into a slot of a linear batch (eval::batch_linear)
inline void batch_set_reference_hlg(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const void *pixels, size_t len, int format,
                                    const HlgDescription &hlg)
{
    detail::check(be, ce_batch_set_reference_hlg(batch, ref_index, pixels, len, format, &hlg), "hlg", 0, 0, 0);
}
inline void batch_set_test_hlg(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len,
                               int format, const HlgDescription &hlg)
{
    detail::check(be, ce_batch_set_test_hlg(batch, pair_index, ref_index, pixels, len, format, &hlg), "hlg", 0, 0, 0);
}
// Y'CbCr planes in HLG, one kernel: yuv_to_rgb16 at depth_out = hlg.depth followed by hlg_to_linear, bit for bit; hlg.depth >= image.depth
inline std::vector<float> yuv_hlg_to_linear(const HipBackend &be, const YuvImage &image, const HlgDescription &hlg, uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_yuv_hlg_to_linear(be.ctx(), &image, &hlg, width, height, out.data(), out.size()), "yuv_hlg", width, height, out.size());
    return out;
}
inline void batch_set_reference_yuv_hlg(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const YuvImage &image, const HlgDescription &hlg)
{
    detail::check(be, ce_batch_set_reference_yuv_hlg(batch, ref_index, &image, &hlg), "yuv_hlg", 0, 0, 0);
}
inline void batch_set_test_yuv_hlg(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const YuvImage &image,
                                   const HlgDescription &hlg)
{
    detail::check(be, ce_batch_set_test_yuv_hlg(batch, pair_index, ref_index, &image, &hlg), "yuv_hlg", 0, 0, 0);
}
// ---- tensors of a framework (include/ce_metrics.h: ce_batch_set_*_tensor) ------------------------------------
// The struct is the ABI's; tensor_chw() / tensor_hwc() fill the two common layouts of `count` contiguous images (NCHW planar;
// NHWC interleaved with `channels` 3 or 4) and the caller changes what differs: a crop's stride_y, a gray tensor's stride_c = 0.
using TensorImage = ce_tensor_image;
inline TensorImage tensor_chw(const void *data, uint32_t width, uint32_t height, int dtype, int memory = CE_MEM_HOST,
                              int quantise = CE_QUANT_NEAREST_EVEN)
{
    TensorImage t{};
    t.data = data, t.dtype = dtype, t.memory = memory, t.quantise = quantise;
    t.stride_x = 1, t.stride_y = width, t.stride_c = (int64_t)width * height, t.stride_n = 3 * t.stride_c;
    return t;
}
inline TensorImage tensor_hwc(const void *data, uint32_t width, uint32_t height, int dtype, int channels = 3, int memory = CE_MEM_HOST,
                              int quantise = CE_QUANT_NEAREST_EVEN)
{
    TensorImage t{};
    t.data = data, t.dtype = dtype, t.memory = memory, t.quantise = quantise;
    t.stride_c = 1, t.stride_x = channels, t.stride_y = (int64_t)width * channels, t.stride_n = t.stride_y * height;
    return t;
}
inline std::vector<uint8_t> tensor_to_rgb8(const HipBackend &be, const TensorImage &t, uint32_t width, uint32_t height)
{
    std::vector<uint8_t> out((size_t)width * height * 3);
    detail::check(be, ce_tensor_to_rgb8(be.ctx(), &t, width, height, out.data(), out.size()), "tensor", width, height, out.size());
    return out;
}
inline std::vector<uint16_t> tensor_to_rgb16(const HipBackend &be, const TensorImage &t, uint32_t width, uint32_t height, uint32_t depth_out)
{
    std::vector<uint16_t> out((size_t)width * height * 3);
    detail::check(be, ce_tensor_to_rgb16(be.ctx(), &t, width, height, depth_out, out.data(), out.size()), "tensor", width, height, out.size());
    return out;
}
inline std::vector<float> tensor_to_linear(const HipBackend &be, const TensorImage &t, uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_tensor_to_linear(be.ctx(), &t, width, height, out.data(), out.size()), "tensor", width, height, out.size());
    return out;
}
// images 0 .. count - 1 into consecutive slots; a device tensor is read in place, behind what the context's stream holds at the call
inline void batch_set_reference_tensor(const HipBackend &be, ce_batch *batch, uint32_t first_ref, uint32_t count, const TensorImage &t)
{
    detail::check(be, ce_batch_set_reference_tensor(batch, first_ref, count, &t), "tensor", 0, 0, 0);
}
inline void batch_set_test_tensor(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const uint32_t *ref_indices, uint32_t count,
                                  const TensorImage &t)
{
    detail::check(be, ce_batch_set_test_tensor(batch, first_pair, ref_indices, count, &t), "tensor", 0, 0, 0);
}
// ---- gain-map images -> their HDR rendition in linear light (include/ce_metrics.h: ce_gainmap_to_linear) ----
// an SDR base image read by a ColourDescription, a small 8-bit map in host memory (the struct carries no length: width *
// height * channels bytes are read) and the metadata, whose gains and headrooms are log2 values
using GainMapImage = ce_gainmap_image;
using GainMapMetadata = ce_gainmap;
// One base image (format: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16; len in bytes) with its map applied -> packed float RGB
inline std::vector<float> gainmap_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, const ColourDescription &colour,
                                            const GainMapImage &map, const GainMapMetadata &metadata, uint32_t width, uint32_t height)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_gainmap_to_linear(be.ctx(), pixels, len, format, &colour, &map, &metadata, width, height, out.data(), out.size()), "gainmap",
                  width, height, len);
    return out;
}
// straight into a slot of a linear batch (eval::batch_linear)
inline void batch_set_reference_gainmap(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const void *pixels, size_t len, int format,
                                        const ColourDescription &colour, const GainMapImage &map, const GainMapMetadata &metadata)
{
    detail::check(be, ce_batch_set_reference_gainmap(batch, ref_index, pixels, len, format, &colour, &map, &metadata), "gainmap", 0, 0, 0);
}
inline void batch_set_test_gainmap(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const void *pixels, size_t len,
                                   int format, const ColourDescription &colour, const GainMapImage &map, const GainMapMetadata &metadata)
{
    detail::check(be, ce_batch_set_test_gainmap(batch, pair_index, ref_index, pixels, len, format, &colour, &map, &metadata), "gainmap", 0, 0, 0);
}
// ---- HDR fidelity of linear batches: PQ-PSNR and BT.2124 Delta E ITP (include/ce_metrics.h: ce_batch_hdr_fidelity) ----
// depth (10, 12 or 16) names the PQ code grid, white_nits the luminance of sample value 1.0
using HdrFidelity = ce_hdr_scores;
// pairs [0, n_pairs) of a linear batch (eval::batch_linear); returns once the scores are on the host
inline std::vector<HdrFidelity> batch_hdr_fidelity(const HipBackend &be, ce_batch *batch, uint32_t n_pairs, uint32_t depth = 10,
                                                   float white_nits = 203.0f)
{
    std::vector<HdrFidelity> out(n_pairs);
    detail::check(be, ce_batch_hdr_fidelity(batch, n_pairs, depth, white_nits, out.data()), "hdr_fidelity", 0, 0, 0);
    return out;
}
// one pair of packed float RGB, linear light with sRGB primaries (width * height * 3 floats each)
inline HdrFidelity hdr_fidelity(const HipBackend &be, const float *reference, const float *test, uint32_t width, uint32_t height,
                                uint32_t depth = 10, float white_nits = 203.0f)
{
    HdrFidelity out{};
    const size_t len = (size_t)width * height * 12;
    detail::check(be, ce_eval_pair_hdr_fidelity(be.ctx(), reference, len, test, len, width, height, depth, white_nits, &out), "hdr_fidelity",
                  width, height, len);
    return out;
}
// Where pairs differ (include/ce_metrics.h: ce_batch_delta_e_itp_map): per pair every pixel's Delta E ITP in
// units of 2^-20 (CE_DELTA_E_ITP_Q20 is 1.0), saturated at 2^32 - 1 - at block 2 .. 64 the maximum of each block x block cell -
// as [count][cells_h][cells_w], empty when want_map is false; and [count][thresholds.size()] counts of the pixels above each
// of up to CE_DELTA_E_ITP_MAX_THRESHOLDS thresholds, empty without thresholds
struct DeltaEItpMaps {
    std::vector<uint32_t> map;
    uint32_t cells_w = 0, cells_h = 0;
    std::vector<uint64_t> over;
    static DeltaEItpMaps sized(uint32_t count, uint32_t width, uint32_t height, uint32_t block, bool want_map, size_t n_thresholds)
    {
        DeltaEItpMaps out;
        const uint32_t b = block ? block : 1;
        out.cells_w = (width + b - 1) / b, out.cells_h = (height + b - 1) / b;
        if (want_map) out.map.resize((size_t)count * out.cells_w * out.cells_h);
        out.over.resize((size_t)count * n_thresholds);
        return out;
    }
};
// pairs [first, first + count) of a linear batch of width x height; returns once the results are on the host
inline DeltaEItpMaps batch_delta_e_itp_map(const HipBackend &be, ce_batch *batch, uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                                           uint32_t depth = 10, float white_nits = 203.0f, uint32_t block = 1, bool want_map = true,
                                           const std::vector<uint32_t> &thresholds_q20 = {})
{
    DeltaEItpMaps out = DeltaEItpMaps::sized(count, width, height, block, want_map, thresholds_q20.size());
    detail::check(be, ce_batch_delta_e_itp_map(batch, first, count, depth, white_nits, block, out.map.empty() ? nullptr : out.map.data(),
                                               out.map.size(), thresholds_q20.empty() ? nullptr : thresholds_q20.data(),
                                               (uint32_t)thresholds_q20.size(), out.over.empty() ? nullptr : out.over.data()),
                  "delta_e_itp_map", 0, 0, 0);
    return out;
}
// one pair of packed float RGB, linear light with sRGB primaries (width * height * 3 floats each)
inline DeltaEItpMaps delta_e_itp_map(const HipBackend &be, const float *reference, const float *test, uint32_t width, uint32_t height,
                                     uint32_t depth = 10, float white_nits = 203.0f, uint32_t block = 1, bool want_map = true,
                                     const std::vector<uint32_t> &thresholds_q20 = {})
{
    DeltaEItpMaps out = DeltaEItpMaps::sized(1, width, height, block, want_map, thresholds_q20.size());
    const size_t len = (size_t)width * height * 12;
    detail::check(be, ce_eval_pair_delta_e_itp_map(be.ctx(), reference, len, test, len, width, height, depth, white_nits, block,
                                                   out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                                   thresholds_q20.empty() ? nullptr : thresholds_q20.data(), (uint32_t)thresholds_q20.size(),
                                                   out.over.empty() ? nullptr : out.over.data()),
                  "delta_e_itp_map", width, height, len);
    return out;
}
// the decision thresholds of PQ code values on linear light, T[1 .. 2^depth - 1] (a pure host function; empty when refused)
inline std::vector<float> pq_code_thresholds(uint32_t depth, float white_nits = 203.0f)
{
    std::vector<float> out(depth == 10 || depth == 12 || depth == 16 ? ((size_t)1 << depth) - 1 : 0);
    if (out.empty() || ce_pq_code_thresholds(depth, white_nits, out.data(), out.size()) != CE_OK) out.clear();
    return out;
}
// the two matrices the kernel is handed, row-major: BT.2020 <- sRGB primaries, BT.2100's LMS <- BT.2020
inline void hdr_fidelity_matrices(std::array<float, 9> &a, std::array<float, 9> &b) { ce_hdr_fidelity_matrices(a.data(), b.data()); }
// ---- SSIM and MS-SSIM on the encoded sample values (include/ce_metrics.h: ce_batch_msssim) ----
// levels: 1 (SSIM) or 5 (MS-SSIM); the struct carries the doubles and the exact integers they are finished from
using MsSsim = ce_msssim_scores;
// pairs [0, n_pairs) of an RGB8 batch or a deep batch of one depth; returns once the scores are on the host
inline std::vector<MsSsim> batch_ms_ssim(const HipBackend &be, ce_batch *batch, uint32_t n_pairs, uint32_t levels = 5)
{
    std::vector<MsSsim> out(n_pairs);
    detail::check(be, ce_batch_msssim(batch, n_pairs, levels, out.data()), "ms_ssim", 0, 0, 0);
    return out;
}
// one pair of packed RGB8 (width * height * 3 bytes each)
inline MsSsim ms_ssim(const HipBackend &be, const uint8_t *reference, const uint8_t *test, uint32_t width, uint32_t height, uint32_t levels = 5)
{
    MsSsim out{};
    const size_t len = (size_t)width * height * 3;
    detail::check(be, ce_eval_pair_msssim(be.ctx(), reference, len, test, len, width, height, levels, &out), "ms_ssim", width, height, len);
    return out;
}
// one pair of packed u16 RGB of `depth` bits on both sides (width * height * 3 samples each)
inline MsSsim ms_ssim_deep(const HipBackend &be, const uint16_t *reference, const uint16_t *test, uint32_t depth, uint32_t width,
                           uint32_t height, uint32_t levels = 5)
{
    MsSsim out{};
    const size_t len = (size_t)width * height * 6;
    detail::check(be, ce_eval_pair_msssim_deep(be.ctx(), reference, len, test, len, depth, width, height, levels, &out), "ms_ssim", width, height,
                  len);
    return out;
}
// ---- CIEDE2000 of RGB8 and deep batches read as sRGB (include/ce_metrics.h: ce_batch_ciede2000) ----
// the struct carries the doubles and the exact integers they are finished from; thresholds_q20: at most eight, in units of 2^-20
using Ciede2000 = ce_ciede2000_scores;
// pairs [0, n_pairs) of an RGB8 or deep batch; returns once the scores are on the host
inline std::vector<Ciede2000> batch_ciede2000(const HipBackend &be, ce_batch *batch, uint32_t n_pairs, const std::vector<uint32_t> &thresholds_q20 = {})
{
    std::vector<Ciede2000> out(n_pairs);
    detail::check(be, ce_batch_ciede2000(batch, n_pairs, thresholds_q20.empty() ? nullptr : thresholds_q20.data(), (uint32_t)thresholds_q20.size(), out.data()),
                  "ciede2000", 0, 0, 0);
    return out;
}
// one pair of packed RGB8 (width * height * 3 bytes each)
inline Ciede2000 ciede2000(const HipBackend &be, const uint8_t *reference, const uint8_t *test, uint32_t width, uint32_t height,
                           const std::vector<uint32_t> &thresholds_q20 = {})
{
    Ciede2000 out{};
    const size_t len = (size_t)width * height * 3;
    detail::check(be, ce_eval_pair_ciede2000(be.ctx(), reference, len, test, len, width, height, thresholds_q20.empty() ? nullptr : thresholds_q20.data(),
                                             (uint32_t)thresholds_q20.size(), &out),
                  "ciede2000", width, height, len);
    return out;
}
// one pair of packed u16 RGB, the reference at ref_depth and the test at test_depth bits (width * height * 3 samples each)
inline Ciede2000 ciede2000_deep(const HipBackend &be, const uint16_t *reference, const uint16_t *test, uint32_t ref_depth, uint32_t test_depth,
                                uint32_t width, uint32_t height, const std::vector<uint32_t> &thresholds_q20 = {})
{
    Ciede2000 out{};
    const size_t len = (size_t)width * height * 6;
    detail::check(be, ce_eval_pair_ciede2000_deep(be.ctx(), reference, len, test, len, ref_depth, test_depth, width, height,
                                                  thresholds_q20.empty() ? nullptr : thresholds_q20.data(), (uint32_t)thresholds_q20.size(), &out),
                  "ciede2000", width, height, len);
    return out;
}
// the per-pixel values in units of 2^-20 of n pixels of packed u16 RGB (a pure host function; empty when refused)
inline std::vector<uint32_t> ciede2000_pixels(const uint16_t *reference, uint32_t ref_depth, const uint16_t *test, uint32_t test_depth, size_t n)
{
    std::vector<uint32_t> out(n);
    if (ce_ciede2000_pixels(reference, ref_depth, test, test_depth, n, out.data()) != CE_OK) out.clear();
    return out;
}
// Where pairs differ and in which direction of colour space (include/ce_metrics.h: ce_batch_ciede2000_map):
// per pair one of a pixel's four values in units of 2^-20 (CE_CIEDE2000_Q20 is 1.0), selected by `what` - CE_CIEDE2000_MAP_DE the
// Delta E 2000 itself, _DL, _DC, _DH the magnitude of its lightness, chroma or hue term, which may exceed the Delta E - at block
// 2 .. 64 the maximum of each block x block cell - as [count][cells_h][cells_w], empty when want_map is false; and
// [count][thresholds.size()] counts of the pixels above each of up to CE_CIEDE2000_MAX_THRESHOLDS thresholds, empty without
// thresholds
struct Ciede2000Maps {
    std::vector<uint32_t> map;
    uint32_t cells_w = 0, cells_h = 0;
    std::vector<uint64_t> over;
    static Ciede2000Maps sized(uint32_t count, uint32_t width, uint32_t height, uint32_t block, bool want_map, size_t n_thresholds)
    {
        Ciede2000Maps out;
        const uint32_t b = block ? block : 1;
        out.cells_w = (width + b - 1) / b, out.cells_h = (height + b - 1) / b;
        if (want_map) out.map.resize((size_t)count * out.cells_w * out.cells_h);
        out.over.resize((size_t)count * n_thresholds);
        return out;
    }
};
// pairs [first, first + count) of an RGB8 or deep batch of width x height; returns once the results are on the host
inline Ciede2000Maps batch_ciede2000_map(const HipBackend &be, ce_batch *batch, uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                                         uint32_t what = CE_CIEDE2000_MAP_DE, uint32_t block = 1, bool want_map = true,
                                         const std::vector<uint32_t> &thresholds_q20 = {})
{
    Ciede2000Maps out = Ciede2000Maps::sized(count, width, height, block, want_map, thresholds_q20.size());
    detail::check(be, ce_batch_ciede2000_map(batch, first, count, what, block, out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                             thresholds_q20.empty() ? nullptr : thresholds_q20.data(), (uint32_t)thresholds_q20.size(),
                                             out.over.empty() ? nullptr : out.over.data()),
                  "ciede2000_map", 0, 0, 0);
    return out;
}
// one pair of packed RGB8 (width * height * 3 bytes each)
inline Ciede2000Maps ciede2000_map(const HipBackend &be, const uint8_t *reference, const uint8_t *test, uint32_t width, uint32_t height,
                                   uint32_t what = CE_CIEDE2000_MAP_DE, uint32_t block = 1, bool want_map = true,
                                   const std::vector<uint32_t> &thresholds_q20 = {})
{
    Ciede2000Maps out = Ciede2000Maps::sized(1, width, height, block, want_map, thresholds_q20.size());
    const size_t len = (size_t)width * height * 3;
    detail::check(be, ce_eval_pair_ciede2000_map(be.ctx(), reference, len, test, len, width, height, what, block,
                                                 out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                                 thresholds_q20.empty() ? nullptr : thresholds_q20.data(), (uint32_t)thresholds_q20.size(),
                                                 out.over.empty() ? nullptr : out.over.data()),
                  "ciede2000_map", width, height, len);
    return out;
}
// one pair of packed u16 RGB, the reference at ref_depth and the test at test_depth bits (width * height * 3 samples each)
inline Ciede2000Maps ciede2000_map_deep(const HipBackend &be, const uint16_t *reference, const uint16_t *test, uint32_t ref_depth,
                                        uint32_t test_depth, uint32_t width, uint32_t height, uint32_t what = CE_CIEDE2000_MAP_DE,
                                        uint32_t block = 1, bool want_map = true, const std::vector<uint32_t> &thresholds_q20 = {})
{
    Ciede2000Maps out = Ciede2000Maps::sized(1, width, height, block, want_map, thresholds_q20.size());
    const size_t len = (size_t)width * height * 6;
    detail::check(be, ce_eval_pair_ciede2000_map_deep(be.ctx(), reference, len, test, len, ref_depth, test_depth, width, height, what, block,
                                                      out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                                      thresholds_q20.empty() ? nullptr : thresholds_q20.data(),
                                                      (uint32_t)thresholds_q20.size(), out.over.empty() ? nullptr : out.over.data()),
                  "ciede2000_map", width, height, len);
    return out;
}
// the four values of n pixels of packed u16 RGB, [n][4] indexed by CE_CIEDE2000_MAP_* (a pure host function; empty when refused)
inline std::vector<uint32_t> ciede2000_pixel_terms(const uint16_t *reference, uint32_t ref_depth, const uint16_t *test, uint32_t test_depth, size_t n)
{
    std::vector<uint32_t> out(n * 4);
    if (ce_ciede2000_pixel_terms(reference, ref_depth, test, test_depth, n, out.data()) != CE_OK) out.clear();
    return out;
}
// the window's eleven literals, and the (width, height) of every level (pure host functions; empty when refused)
inline std::array<double, 11> msssim_window()
{
    std::array<double, 11> g{};
    ce_msssim_window(g.data());
    return g;
}
inline std::vector<std::pair<uint32_t, uint32_t>> msssim_levels(uint32_t width, uint32_t height, uint32_t levels = 5)
{
    uint32_t n = 0, w[CE_MSSSIM_LEVELS], h[CE_MSSSIM_LEVELS];
    std::vector<std::pair<uint32_t, uint32_t>> out;
    if (ce_msssim_levels(width, height, levels, &n, w, h) != CE_OK) return out;
    for (uint32_t l = 0; l < n; l++) out.emplace_back(w[l], h[l]);
    return out;
}
// Where pairs differ at one level of the pyramid (include/ce_metrics.h: ce_batch_msssim_map): per pair and
// channel every valid position's 2^32 - q in units of 2^-32 (CE_MSSSIM_Q32 is an SSIM of 1.0), q the integer ms_ssim sums - of
// SSIM (CE_MSSSIM_MAP_SSIM) or of the contrast-structure term (CE_MSSSIM_MAP_CS) - saturated to [0, 2^32 - 1]; at block 2 .. 64
// the maximum of each block x block cell - as [count][3][cells_h][cells_w], empty when want_map is false; and [count][3]
// [thresholds.size()] counts of the positions above each of up to CE_MSSSIM_MAP_MAX_THRESHOLDS thresholds, empty without
// thresholds.  What the library refuses (levels, level, an image too small) leaves the map empty for it to refuse.
struct MsSsimMaps {
    std::vector<uint32_t> map;
    uint32_t cells_w = 0, cells_h = 0;
    std::vector<uint64_t> over;
    static MsSsimMaps sized(uint32_t count, uint32_t width, uint32_t height, uint32_t levels, uint32_t level, uint32_t block, bool want_map,
                            size_t n_thresholds)
    {
        MsSsimMaps out;
        const uint32_t b = block ? block : 1;
        const auto lv = msssim_levels(width, height, levels);
        if (level < lv.size()) out.cells_w = (lv[level].first - 10 + b - 1) / b, out.cells_h = (lv[level].second - 10 + b - 1) / b;
        if (want_map) out.map.resize((size_t)count * 3 * out.cells_w * out.cells_h);
        out.over.resize((size_t)count * 3 * n_thresholds);
        return out;
    }
};
// pairs [first, first + count) of an RGB8 batch or a deep batch of one depth, of width x height; returns once the results are on the host
inline MsSsimMaps batch_ms_ssim_map(const HipBackend &be, ce_batch *batch, uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                                    uint32_t levels = 5, uint32_t level = 0, uint32_t what = CE_MSSSIM_MAP_SSIM, uint32_t block = 1,
                                    bool want_map = true, const std::vector<uint32_t> &thresholds_q32 = {})
{
    MsSsimMaps out = MsSsimMaps::sized(count, width, height, levels, level, block, want_map, thresholds_q32.size());
    detail::check(be, ce_batch_msssim_map(batch, first, count, levels, level, what, block, out.map.empty() ? nullptr : out.map.data(),
                                          out.map.size(), thresholds_q32.empty() ? nullptr : thresholds_q32.data(),
                                          (uint32_t)thresholds_q32.size(), out.over.empty() ? nullptr : out.over.data()),
                  "ms_ssim_map", 0, 0, 0);
    return out;
}
// one pair of packed RGB8 (width * height * 3 bytes each)
inline MsSsimMaps ms_ssim_map(const HipBackend &be, const uint8_t *reference, const uint8_t *test, uint32_t width, uint32_t height,
                              uint32_t levels = 5, uint32_t level = 0, uint32_t what = CE_MSSSIM_MAP_SSIM, uint32_t block = 1,
                              bool want_map = true, const std::vector<uint32_t> &thresholds_q32 = {})
{
    MsSsimMaps out = MsSsimMaps::sized(1, width, height, levels, level, block, want_map, thresholds_q32.size());
    const size_t len = (size_t)width * height * 3;
    detail::check(be, ce_eval_pair_msssim_map(be.ctx(), reference, len, test, len, width, height, levels, level, what, block,
                                              out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                              thresholds_q32.empty() ? nullptr : thresholds_q32.data(), (uint32_t)thresholds_q32.size(),
                                              out.over.empty() ? nullptr : out.over.data()),
                  "ms_ssim_map", width, height, len);
    return out;
}
// one pair of packed u16 RGB of `depth` bits on both sides (width * height * 3 samples each)
inline MsSsimMaps ms_ssim_map_deep(const HipBackend &be, const uint16_t *reference, const uint16_t *test, uint32_t depth, uint32_t width,
                                   uint32_t height, uint32_t levels = 5, uint32_t level = 0, uint32_t what = CE_MSSSIM_MAP_SSIM,
                                   uint32_t block = 1, bool want_map = true, const std::vector<uint32_t> &thresholds_q32 = {})
{
    MsSsimMaps out = MsSsimMaps::sized(1, width, height, levels, level, block, want_map, thresholds_q32.size());
    const size_t len = (size_t)width * height * 6;
    detail::check(be, ce_eval_pair_msssim_map_deep(be.ctx(), reference, len, test, len, depth, width, height, levels, level, what, block,
                                                   out.map.empty() ? nullptr : out.map.data(), out.map.size(),
                                                   thresholds_q32.empty() ? nullptr : thresholds_q32.data(), (uint32_t)thresholds_q32.size(),
                                                   out.over.empty() ? nullptr : out.over.data()),
                  "ms_ssim_map", width, height, len);
    return out;
}
// ---- a decoder's Y'CbCr planes scored as planes (include/ce_metrics.h: ce_yuv_plane_fidelity) ----
// PSNR-Y / -Cb / -Cr with the weighted and the overall figure, and SSIM / MS-SSIM per plane, each plane at its own size;
// levels: 0 (PSNR only), 1 (+ SSIM) or 5 (+ MS-SSIM)
using PlaneScores = ce_plane_scores;
// tests[i] against refs[pair_ref[i]], or against refs[i] with an empty pair_ref (then refs.size() == tests.size()); host or
// device planes, every image width x height with one subsampling and one depth; returns once the scores are on the host
inline std::vector<PlaneScores> plane_fidelity(const HipBackend &be, const std::vector<ce_yuv_image> &refs, const std::vector<ce_yuv_image> &tests,
                                               uint32_t width, uint32_t height, const std::vector<uint32_t> &pair_ref = {}, uint32_t levels = 5)
{
    std::vector<PlaneScores> out(tests.size());
    if (!pair_ref.empty() && pair_ref.size() != tests.size()) detail::check(be, CE_ERR_INVALID_ARG, "plane_fidelity", width, height, 0);
    detail::check(be, ce_yuv_plane_fidelity(be.ctx(), width, height, refs.data(), (uint32_t)refs.size(), tests.data(), (uint32_t)tests.size(),
                                            pair_ref.empty() ? nullptr : pair_ref.data(), levels, out.data()),
                  "plane_fidelity", width, height, 0);
    return out;
}
// ---- PSNR-HVS and PSNR-HVS-M of the same planes (include/ce_metrics.h: ce_yuv_plane_hvs) ----
// per plane the two exact sums, the block count and the two scores; step: samples from a DCT block to the next, 1 .. 8
using PlaneHvsScores = ce_plane_hvs_scores;
inline std::vector<PlaneHvsScores> plane_hvs(const HipBackend &be, const std::vector<ce_yuv_image> &refs, const std::vector<ce_yuv_image> &tests,
                                             uint32_t width, uint32_t height, const std::vector<uint32_t> &pair_ref = {}, uint32_t step = 8)
{
    std::vector<PlaneHvsScores> out(tests.size());
    if (!pair_ref.empty() && pair_ref.size() != tests.size()) detail::check(be, CE_ERR_INVALID_ARG, "plane_hvs", width, height, 0);
    detail::check(be, ce_yuv_plane_hvs(be.ctx(), width, height, refs.data(), (uint32_t)refs.size(), tests.data(), (uint32_t)tests.size(),
                                       pair_ref.empty() ? nullptr : pair_ref.data(), step, out.data()),
                  "plane_hvs", width, height, 0);
    return out;
}
// ---- pixel-domain VIF (VIFp) of the same planes (include/ce_metrics.h: ce_yuv_plane_vif) ----
// per plane and scale the two exact sums in units of 2^-24 nat, the positions, their ratio, and vifp over the four scales
using PlaneVifScores = ce_plane_vif_scores;
inline std::vector<PlaneVifScores> plane_vif(const HipBackend &be, const std::vector<ce_yuv_image> &refs, const std::vector<ce_yuv_image> &tests,
                                             uint32_t width, uint32_t height, const std::vector<uint32_t> &pair_ref = {})
{
    std::vector<PlaneVifScores> out(tests.size());
    if (!pair_ref.empty() && pair_ref.size() != tests.size()) detail::check(be, CE_ERR_INVALID_ARG, "plane_vif", width, height, 0);
    detail::check(be, ce_yuv_plane_vif(be.ctx(), width, height, refs.data(), (uint32_t)refs.size(), tests.data(), (uint32_t)tests.size(),
                                       pair_ref.empty() ? nullptr : pair_ref.data(), out.data()),
                  "plane_vif", width, height, 0);
    return out;
}
// the 17, 9, 5 or 3 literals of scale 1 .. 4's window (a pure host function; empty when refused)
inline std::vector<double> vif_window(uint32_t scale)
{
    std::vector<double> g(17);
    if (ce_vif_window(scale, g.data()) != CE_OK) return {};
    g.resize(scale == 1 ? 17 : scale == 2 ? 9 : scale == 3 ? 5 : 3);
    return g;
}
// ---- GMSD of the same planes (include/ce_metrics.h: ce_yuv_plane_gmsd) ----
// per plane the exact sum of the similarities in units of 2^-32, the exact sum of their squares as [low, high] 64 bits, the
// positions, the deviation (dividing by N), the mean and the largest 2^32 - q
using PlaneGmsdScores = ce_plane_gmsd_scores;
inline std::vector<PlaneGmsdScores> plane_gmsd(const HipBackend &be, const std::vector<ce_yuv_image> &refs, const std::vector<ce_yuv_image> &tests,
                                               uint32_t width, uint32_t height, const std::vector<uint32_t> &pair_ref = {})
{
    std::vector<PlaneGmsdScores> out(tests.size());
    if (!pair_ref.empty() && pair_ref.size() != tests.size()) detail::check(be, CE_ERR_INVALID_ARG, "plane_gmsd", width, height, 0);
    detail::check(be, ce_yuv_plane_gmsd(be.ctx(), width, height, refs.data(), (uint32_t)refs.size(), tests.data(), (uint32_t)tests.size(),
                                        pair_ref.empty() ? nullptr : pair_ref.data(), out.data()),
                  "plane_gmsd", width, height, 0);
    return out;
}
// straight into a slot of a resident batch (RGB8 or deep), host or device planes
inline void batch_set_reference_yuv(const HipBackend &be, ce_batch *batch, uint32_t ref_index, const YuvImage &image)
{
    detail::check(be, ce_batch_set_reference_yuv(batch, ref_index, &image), "yuv", 0, 0, 0);
}
inline void batch_set_test_yuv(const HipBackend &be, ce_batch *batch, uint32_t pair_index, uint32_t ref_index, const YuvImage &image)
{
    detail::check(be, ce_batch_set_test_yuv(batch, pair_index, ref_index, &image), "yuv", 0, 0, 0);
}

// ---- alpha: a transparent image composited over solid backgrounds on the device -----------------
// straight alpha, source-over onto an opaque colour, on the encoded values: (c a + bg (m - a) + (m >> 1)) / m
using Background = std::array<uint16_t, 3>;  // samples at the destination's depth (8-bit: <= 255)
inline Bytes composite_rgba8(const HipBackend &be, const Bytes &rgba, uint32_t width, uint32_t height, const std::array<uint8_t, 3> &background)
{
    Bytes out((size_t)width * height * 3);
    detail::check(be, ce_composite_rgba8(be.ctx(), rgba.data(), rgba.size(), width, height, background.data(), out.data(), out.size()),
                  "alpha", width, height, rgba.size());
    return out;
}
inline std::vector<uint16_t> composite_rgba16(const HipBackend &be, const std::vector<uint16_t> &rgba, uint32_t width, uint32_t height,
                                              uint32_t depth, const Background &background)
{
    std::vector<uint16_t> out((size_t)width * height * 3);
    detail::check(be, ce_composite_rgba16(be.ctx(), rgba.data(), rgba.size(), width, height, depth, background.data(), out.data(), out.size()),
                  "alpha", width, height, rgba.size());
    return out;
}
// one upload into backgrounds.size() consecutive slots of a resident batch (RGB8 or deep), slot k over backgrounds[k]
inline void batch_set_reference_over(const HipBackend &be, ce_batch *batch, uint32_t first_ref, const void *pixels, size_t len, int format,
                                     const std::vector<Background> &backgrounds)
{
    detail::check(be, ce_batch_set_reference_over(batch, first_ref, pixels, len, format, (uint32_t)backgrounds.size(),
                                                  backgrounds.empty() ? nullptr : backgrounds[0].data()), "alpha", 0, 0, len);
}
inline void batch_set_test_over(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const std::vector<uint32_t> &ref_indices,
                                const void *pixels, size_t len, int format, const std::vector<Background> &backgrounds)
{
    if (ref_indices.size() != backgrounds.size()) throw Error(Error::Kind::MetricCalculation, "alpha: one reference index per background");
    detail::check(be, ce_batch_set_test_over(batch, first_pair, ref_indices.data(), pixels, len, format, (uint32_t)backgrounds.size(),
                                             backgrounds.empty() ? nullptr : backgrounds[0].data()), "alpha", 0, 0, len);
}

// ---- alpha in linear light: the pixel turned into linear light, then blended over solid colours ---------
// o = (t == 1) ? v : (t == 0) ? bg : (v t) + (bg (1 - t)) in separately rounded f32; include/ce_metrics.h holds the definition
using LinearBackground = std::array<float, 3>;  // linear light, sRGB primaries, finite and within +-CE_LINEAR_MAX
inline std::vector<float> alpha_table(uint32_t depth)
{
    std::vector<float> out(depth <= 16 ? (size_t)1 << depth : 1);
    if (ce_alpha_table(depth, out.data(), out.size()) != CE_OK) throw Error(Error::Kind::MetricCalculation, ce_last_error(nullptr));
    return out;
}
inline const float *linear_bg_data(const std::vector<LinearBackground> &b) { return b.empty() ? nullptr : b[0].data(); }
inline void one_ref_per_background(const std::vector<uint32_t> &refs, const std::vector<LinearBackground> &b)
{
    if (refs.size() != b.size()) throw Error(Error::Kind::MetricCalculation, "alpha: one reference index per background");
}
// one image over one background to packed float RGB in host memory
inline std::vector<float> cicp_over_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, const ColourDescription &colour,
                                              uint32_t width, uint32_t height, const LinearBackground &background)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_cicp_over_to_linear(be.ctx(), pixels, len, format, &colour, width, height, background.data(), out.data(), out.size()),
                  "alpha", width, height, len);
    return out;
}
inline std::vector<float> hlg_over_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, const HlgDescription &hlg,
                                             uint32_t width, uint32_t height, const LinearBackground &background)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_hlg_over_to_linear(be.ctx(), pixels, len, format, &hlg, width, height, background.data(), out.data(), out.size()),
                  "alpha", width, height, len);
    return out;
}
inline std::vector<float> icc_over_to_linear(const HipBackend &be, const void *pixels, size_t len, int format, uint32_t depth,
                                             const HipIccProfile &icc, uint32_t width, uint32_t height, const LinearBackground &background)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_icc_over_to_linear(be.ctx(), pixels, len, format, depth, icc.get(), width, height, background.data(), out.data(), out.size()),
                  "alpha", width, height, len);
    return out;
}
inline std::vector<float> linear_over(const HipBackend &be, const std::vector<float> &rgba, bool premultiplied, uint32_t width, uint32_t height,
                                      const LinearBackground &background)
{
    std::vector<float> out((size_t)width * height * 3);
    detail::check(be, ce_linear_over(be.ctx(), rgba.data(), rgba.size() * sizeof(float), CE_PIXEL_RGBA_F32, premultiplied, width, height,
                                     background.data(), out.data(), out.size()), "alpha", width, height, rgba.size() * sizeof(float));
    return out;
}
// one upload into backgrounds.size() consecutive slots of a linear batch, slot k over backgrounds[k]
inline void batch_set_reference_cicp_over(const HipBackend &be, ce_batch *batch, uint32_t first_ref, const void *pixels, size_t len, int format,
                                          const ColourDescription &colour, const std::vector<LinearBackground> &backgrounds)
{
    detail::check(be, ce_batch_set_reference_cicp_over(batch, first_ref, pixels, len, format, &colour, (uint32_t)backgrounds.size(),
                                                       linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_test_cicp_over(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const std::vector<uint32_t> &ref_indices,
                                     const void *pixels, size_t len, int format, const ColourDescription &colour,
                                     const std::vector<LinearBackground> &backgrounds)
{
    one_ref_per_background(ref_indices, backgrounds);
    detail::check(be, ce_batch_set_test_cicp_over(batch, first_pair, ref_indices.data(), pixels, len, format, &colour, (uint32_t)backgrounds.size(),
                                                  linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_reference_hlg_over(const HipBackend &be, ce_batch *batch, uint32_t first_ref, const void *pixels, size_t len, int format,
                                         const HlgDescription &hlg, const std::vector<LinearBackground> &backgrounds)
{
    detail::check(be, ce_batch_set_reference_hlg_over(batch, first_ref, pixels, len, format, &hlg, (uint32_t)backgrounds.size(),
                                                      linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_test_hlg_over(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const std::vector<uint32_t> &ref_indices,
                                    const void *pixels, size_t len, int format, const HlgDescription &hlg,
                                    const std::vector<LinearBackground> &backgrounds)
{
    one_ref_per_background(ref_indices, backgrounds);
    detail::check(be, ce_batch_set_test_hlg_over(batch, first_pair, ref_indices.data(), pixels, len, format, &hlg, (uint32_t)backgrounds.size(),
                                                 linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_reference_icc_over(const HipBackend &be, ce_batch *batch, uint32_t first_ref, const void *pixels, size_t len, int format,
                                         uint32_t depth, const HipIccProfile &icc, const std::vector<LinearBackground> &backgrounds)
{
    detail::check(be, ce_batch_set_reference_icc_over(batch, first_ref, pixels, len, format, depth, icc.get(), (uint32_t)backgrounds.size(),
                                                      linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_test_icc_over(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const std::vector<uint32_t> &ref_indices,
                                    const void *pixels, size_t len, int format, uint32_t depth, const HipIccProfile &icc,
                                    const std::vector<LinearBackground> &backgrounds)
{
    one_ref_per_background(ref_indices, backgrounds);
    detail::check(be, ce_batch_set_test_icc_over(batch, first_pair, ref_indices.data(), pixels, len, format, depth, icc.get(),
                                                 (uint32_t)backgrounds.size(), linear_bg_data(backgrounds)), "alpha", 0, 0, len);
}
inline void batch_set_reference_linear_over(const HipBackend &be, ce_batch *batch, uint32_t first_ref, const std::vector<float> &rgba,
                                            bool premultiplied, const std::vector<LinearBackground> &backgrounds)
{
    detail::check(be, ce_batch_set_reference_linear_over(batch, first_ref, rgba.data(), rgba.size() * sizeof(float), CE_PIXEL_RGBA_F32, premultiplied,
                                                         (uint32_t)backgrounds.size(), linear_bg_data(backgrounds)), "alpha", 0, 0, rgba.size() * 4);
}
inline void batch_set_test_linear_over(const HipBackend &be, ce_batch *batch, uint32_t first_pair, const std::vector<uint32_t> &ref_indices,
                                       const std::vector<float> &rgba, bool premultiplied, const std::vector<LinearBackground> &backgrounds)
{
    one_ref_per_background(ref_indices, backgrounds);
    detail::check(be, ce_batch_set_test_linear_over(batch, first_pair, ref_indices.data(), rgba.data(), rgba.size() * sizeof(float), CE_PIXEL_RGBA_F32,
                                                    premultiplied, (uint32_t)backgrounds.size(), linear_bg_data(backgrounds)), "alpha", 0, 0,
                  rgba.size() * 4);
}
}  // namespace metrics

namespace eval {

// ---- src/eval/session.rs:25-147 (the slice variants; imgref variants collapse to them in C++) ----------
struct ImageData {
    enum class Format { Rgb8, Rgba8 } format = Format::Rgb8;
    std::vector<uint8_t> data;
    size_t width = 0, height = 0;
    std::optional<std::vector<uint8_t>> icc_profile;  // RgbSliceWithIcc, session.rs:60-77
    static ImageData rgb(std::vector<uint8_t> d, size_t w, size_t h) { return {Format::Rgb8, std::move(d), w, h, std::nullopt}; }
    static ImageData rgba(std::vector<uint8_t> d, size_t w, size_t h) { return {Format::Rgba8, std::move(d), w, h, std::nullopt}; }
    static ImageData rgb_with_icc(std::vector<uint8_t> d, size_t w, size_t h, std::vector<uint8_t> icc)
    {
        return {Format::Rgb8, std::move(d), w, h, std::move(icc)};
    }
    // to_rgb8_vec, session.rs:98-117: alpha is dropped
    std::vector<uint8_t> to_rgb8_vec() const
    {
        if (format == Format::Rgb8) return data;
        std::vector<uint8_t> out;
        out.reserve(width * height * 3);
        for (size_t i = 0; i + 3 < data.size(); i += 4) out.insert(out.end(), {data[i], data[i + 1], data[i + 2]});
        return out;
    }
};

// ---- ICC -> sRGB (src/metrics/icc.rs:69-103) as a device colour table --------------------------------------------------
// Cms: the host's colour management, 8-bit RGB -> 8-bit RGB for one profile (the reference's default build uses moxcms).
// It is evaluated once per profile on the identity colour cube; the table then lives on the device (ce_lut_*).
using Cms = std::function<std::vector<uint8_t>(const std::vector<uint8_t> &icc_profile, const std::vector<uint8_t> &rgb)>;

class HipColorTable {
public:
    HipColorTable(const HipBackend &be, const Cms &cms, const std::vector<uint8_t> &icc_profile)
    {
        std::vector<uint8_t> cube((size_t)3 << 24);
        for (uint32_t v = 0; v < (1u << 24); v++) {
            cube[3 * (size_t)v] = (uint8_t)(v >> 16);
            cube[3 * (size_t)v + 1] = (uint8_t)(v >> 8);
            cube[3 * (size_t)v + 2] = (uint8_t)v;
        }
        const std::vector<uint8_t> table = cms(icc_profile, cube);
        if (ce_lut_create(be.ctx(), table.data(), table.size(), &lut_) != CE_OK)
            throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: ICC: Failed to create ICC transform: " + be.last_error());
    }
    ~HipColorTable() { ce_lut_destroy(lut_); }
    HipColorTable(const HipColorTable &) = delete;
    HipColorTable &operator=(const HipColorTable &) = delete;
    const ce_lut *get() const { return lut_; }

private:
    ce_lut *lut_ = nullptr;
};

struct EncodeRequest {  // session.rs:151-177
    double quality = 0;
    std::map<std::string, std::string> params;
};
using EncodeFn = std::function<std::vector<uint8_t>(const ImageData &, const EncodeRequest &)>;  // session.rs:181
using DecodeFn = std::function<ImageData(const std::vector<uint8_t> &)>;                          // session.rs:186

struct EvalConfig {  // session.rs:190-279; the default quality sweep is :273-275
    MetricConfig metrics = MetricConfig::all();
    std::vector<double> quality_levels = {50.0, 60.0, 70.0, 80.0, 85.0, 90.0, 95.0};
    float intensity_target = CE_DEFAULT_INTENSITY_TARGET;
    // session.rs:196 carries the condition and nothing reads it.  simulate_viewing unset: every score is what it always was.
    // Set: the source and every decode are resampled on the device to the size `viewing` displays them at
    // (SimulationParams::displayed_size) and scored there; untagged (sRGB) decodes only.
    viewing::ViewingCondition viewing;
    std::optional<viewing::SimulationMode> simulate_viewing;
    int resample_filter = CE_RESAMPLE_LANCZOS3;
    // Not in the reference, which drops alpha (session.rs:98-117).  Empty: every score is what it always was.  8-bit colours
    // (kAlphaBlackWhite): a pair whose source or decode is Rgba8 is composited over each on the device and scored over each;
    // CodecResult::metrics carries the worst value per metric, ImageReport::alpha_scores the per-background ones.
    std::vector<std::array<uint8_t, 3>> alpha_backgrounds;
};
inline const std::vector<std::array<uint8_t, 3>> kAlphaBlackWhite = {{0, 0, 0}, {255, 255, 255}};

// one pair's scores over each background -> the worst value per metric: max DSSIM, max Butteraugli, min SSIMULACRA2, min PSNR
inline MetricResult worst_over_backgrounds(const std::vector<MetricResult> &per_bg)
{
    MetricResult w = per_bg.at(0);
    for (size_t k = 1; k < per_bg.size(); k++) {
        const MetricResult &m = per_bg[k];
        w.dssim = w.dssim && m.dssim ? std::optional<double>(std::max(*w.dssim, *m.dssim)) : std::nullopt;
        w.butteraugli = w.butteraugli && m.butteraugli ? std::optional<double>(std::max(*w.butteraugli, *m.butteraugli)) : std::nullopt;
        w.ssimulacra2 = w.ssimulacra2 && m.ssimulacra2 ? std::optional<double>(std::min(*w.ssimulacra2, *m.ssimulacra2)) : std::nullopt;
        w.psnr = w.psnr && m.psnr ? std::optional<double>(std::min(*w.psnr, *m.psnr)) : std::nullopt;
    }
    return w;
}

struct CodecResult {  // src/eval/report.rs:16-52
    std::string codec_id, codec_version;
    double quality = 0;
    size_t file_size = 0;
    double bits_per_pixel = 0;
    std::chrono::nanoseconds encode_time{0};
    std::optional<std::chrono::nanoseconds> decode_time;
    MetricResult metrics;
    std::optional<PerceptionLevel> perception;
    std::map<std::string, std::string> codec_params;
};
struct ImageReport {  // report.rs:68-136
    std::string name;
    uint32_t width = 0, height = 0;
    std::vector<CodecResult> results;
    // EvalConfig::alpha_backgrounds: result index -> its scores over each background, for the results that were composited
    std::map<size_t, std::vector<MetricResult>> alpha_scores;
};

class EvalSession {  // session.rs:281-497
public:
    EvalSession(std::shared_ptr<HipBackend> backend, EvalConfig config) : be_(std::move(backend)), config_(std::move(config)) {}
    EvalSession &add_codec(std::string id, std::string version, EncodeFn encode)
    {
        codecs_.push_back({std::move(id), std::move(version), std::move(encode), nullptr});
        return *this;
    }
    EvalSession &add_codec_with_decode(std::string id, std::string version, EncodeFn encode, DecodeFn decode)
    {
        codecs_.push_back({std::move(id), std::move(version), std::move(encode), std::move(decode)});
        return *this;
    }
    size_t codec_count() const { return codecs_.size(); }
    // the host's ICC -> sRGB transform for tagged DECODED images (session.rs:394); without one a tagged image fails like
    // a build without the `icc` feature (icc.rs:105-113).  Tables are built once per distinct profile and kept.
    EvalSession &set_cms(Cms cms)
    {
        cms_ = std::move(cms);
        return *this;
    }

    // evaluate_image, session.rs:368-434
    ImageReport evaluate_image(const std::string &name, const ImageData &image) const
    {
        std::vector<const ce_lut *> luts;
        ImageReport report{name, (uint32_t)image.width, (uint32_t)image.height, {}, {}};
        if (!config_.alpha_backgrounds.empty()) return evaluate_image_over(std::move(report), image);
        const std::vector<uint8_t> reference_rgb = image.to_rgb8_vec();
        std::vector<std::vector<uint8_t>> decoded;  // kept alive until the batch has run
        std::vector<size_t> result_of_pair;
        decoded.reserve(codecs_.size() * config_.quality_levels.size());
        for (const auto &codec : codecs_)
            for (double quality : config_.quality_levels) {
                EncodeRequest request{quality, {}};
                const auto t0 = std::chrono::steady_clock::now();
                const std::vector<uint8_t> encoded = codec.encode(image, request);
                const auto t1 = std::chrono::steady_clock::now();
                CodecResult r;
                r.codec_id = codec.id;
                r.codec_version = codec.version;
                r.quality = quality;
                r.file_size = encoded.size();
                r.bits_per_pixel = (double)(encoded.size() * 8) / ((double)image.width * (double)image.height);
                r.encode_time = t1 - t0;
                r.codec_params = request.params;
                if (codec.decode) {
                    const auto d0 = std::chrono::steady_clock::now();
                    const ImageData dec = codec.decode(encoded);
                    r.decode_time = std::chrono::steady_clock::now() - d0;
                    decoded.push_back(dec.to_rgb8_vec());
                    luts.push_back(table_for(dec));  // to_rgb8_srgb (session.rs:394) runs on the device
                    result_of_pair.push_back(report.results.size());
                }
                report.results.push_back(std::move(r));
            }
        if (!decoded.empty()) {
            uint32_t sw = (uint32_t)image.width, sh = (uint32_t)image.height;
            std::vector<uint8_t> shown_reference;
            const std::vector<uint8_t> *ref = &reference_rgb;
            if (config_.simulate_viewing) {
                const auto shown = config_.viewing.simulation_params(sw, sh, *config_.simulate_viewing).displayed_size(sw, sh);
                if (shown != std::make_pair(sw, sh)) {
                    for (const ce_lut *lut : luts)
                        if (lut) throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: viewing simulation takes untagged (sRGB) decodes only");
                    shown_reference = metrics::resample_rgb8(*be_, reference_rgb, sw, sh, shown.first, shown.second, config_.resample_filter);
                    ref = &shown_reference;
                    for (auto &d : decoded) {
                        detail::check(*be_, d.size() == reference_rgb.size() ? CE_OK : CE_ERR_DIM_MISMATCH, "metric", sw, sh, d.size());
                        d = metrics::resample_rgb8(*be_, d, sw, sh, shown.first, shown.second, config_.resample_filter);
                    }
                    sw = shown.first, sh = shown.second;
                }
            }
            std::vector<ce_pair_desc> pairs(decoded.size());
            for (size_t i = 0; i < decoded.size(); i++)
                pairs[i] = {ref->data(), ref->size(), decoded[i].data(), decoded[i].size(), sw, sh};
            std::vector<ce_scores> scores(decoded.size());
            const int rc = ce_eval_batch_lut(be_->ctx(), pairs.size(), pairs.data(), luts.data(), config_.metrics.mask(),
                                             config_.metrics.flags(), config_.intensity_target, scores.data());
            detail::check(*be_, rc, "batch", image.width, image.height, reference_rgb.size());
            for (size_t i = 0; i < decoded.size(); i++) {
                detail::check(*be_, scores[i].status, "metric", image.width, image.height, decoded[i].size());  // `?` in :394-396
                CodecResult &r = report.results[result_of_pair[i]];
                r.metrics = MetricResult::from_c(scores[i]);
                r.perception = r.metrics.perception_level();  // session.rs:407
            }
        }
        return report;
    }

private:
    struct CodecEntry {
        std::string id, version;
        EncodeFn encode;
        DecodeFn decode;
    };
    // `image` seen over `bg`: composited on the device (ce_composite_rgba8) if it has alpha, to_rgb8_vec otherwise
    std::vector<uint8_t> seen_over(const ImageData &image, const std::array<uint8_t, 3> &bg) const
    {
        if (image.format != ImageData::Format::Rgba8) return image.to_rgb8_vec();
        return metrics::composite_rgba8(*be_, image.data, (uint32_t)image.width, (uint32_t)image.height, bg);
    }
    // evaluate_image with EvalConfig::alpha_backgrounds set: the sweep as ever; a pair with alpha on either side becomes one
    // pair per background of the pooled batch call, a pair without stays one
    ImageReport evaluate_image_over(ImageReport report, const ImageData &image) const
    {
        if (config_.simulate_viewing) throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: alpha_backgrounds with simulate_viewing is not offered here");
        const auto &bgs = config_.alpha_backgrounds;
        const bool src_alpha = image.format == ImageData::Format::Rgba8;
        std::vector<std::vector<uint8_t>> refs;  // the source over each background (one entry if it has no alpha)
        for (size_t k = 0; k < (src_alpha ? bgs.size() : 1); k++) refs.push_back(seen_over(image, bgs[k]));
        std::vector<std::vector<uint8_t>> tests;
        std::vector<const ce_lut *> luts;
        std::vector<size_t> ref_of_pair, result_of_pair;
        for (const auto &codec : codecs_)
            for (double quality : config_.quality_levels) {
                EncodeRequest request{quality, {}};
                const auto t0 = std::chrono::steady_clock::now();
                const std::vector<uint8_t> encoded = codec.encode(image, request);
                const auto t1 = std::chrono::steady_clock::now();
                CodecResult r;
                r.codec_id = codec.id;
                r.codec_version = codec.version;
                r.quality = quality;
                r.file_size = encoded.size();
                r.bits_per_pixel = (double)(encoded.size() * 8) / ((double)image.width * (double)image.height);
                r.encode_time = t1 - t0;
                r.codec_params = request.params;
                if (codec.decode) {
                    const auto d0 = std::chrono::steady_clock::now();
                    const ImageData dec = codec.decode(encoded);
                    r.decode_time = std::chrono::steady_clock::now() - d0;
                    const bool dec_alpha = dec.format == ImageData::Format::Rgba8;
                    const ce_lut *lut = table_for(dec);
                    if (dec_alpha && lut) throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: alpha_backgrounds: a decode with alpha and an ICC profile is not supported");
                    if (dec_alpha && (dec.width != image.width || dec.height != image.height))
                        detail::check(*be_, CE_ERR_DIM_MISMATCH, "metric", image.width, image.height, dec.data.size());
                    for (size_t k = 0; k < (src_alpha || dec_alpha ? bgs.size() : 1); k++) {
                        tests.push_back(seen_over(dec, bgs[k]));
                        luts.push_back(lut);
                        ref_of_pair.push_back(src_alpha ? k : 0);
                        result_of_pair.push_back(report.results.size());
                    }
                }
                report.results.push_back(std::move(r));
            }
        if (tests.empty()) return report;
        std::vector<ce_pair_desc> pairs(tests.size());
        for (size_t i = 0; i < tests.size(); i++) {
            const auto &ref = refs[ref_of_pair[i]];
            pairs[i] = {ref.data(), ref.size(), tests[i].data(), tests[i].size(), (uint32_t)image.width, (uint32_t)image.height};
        }
        std::vector<ce_scores> scores(tests.size());
        const int rc = ce_eval_batch_lut(be_->ctx(), pairs.size(), pairs.data(), luts.data(), config_.metrics.mask(), config_.metrics.flags(),
                                         config_.intensity_target, scores.data());
        detail::check(*be_, rc, "batch", image.width, image.height, refs[0].size());
        std::map<size_t, std::vector<MetricResult>> per_result;
        for (size_t i = 0; i < tests.size(); i++) {
            detail::check(*be_, scores[i].status, "metric", image.width, image.height, tests[i].size());
            per_result[result_of_pair[i]].push_back(MetricResult::from_c(scores[i]));
        }
        for (auto &[index, per_bg] : per_result) {
            CodecResult &r = report.results[index];
            r.metrics = worst_over_backgrounds(per_bg);
            r.perception = r.metrics.perception_level();  // session.rs:407
            if (per_bg.size() > 1) report.alpha_scores[index] = std::move(per_bg);
        }
        return report;
    }
    const ce_lut *table_for(const ImageData &decoded) const
    {
        if (!decoded.icc_profile) return nullptr;  // ColorProfile::Srgb: a plain copy (icc.rs:73)
        if (!cms_)
            throw Error(Error::Kind::MetricCalculation, "Metric calculation failed: ICC: ICC profile support requires the 'icc' feature");
        auto it = tables_.find(*decoded.icc_profile);
        if (it == tables_.end()) it = tables_.emplace(*decoded.icc_profile, std::make_unique<HipColorTable>(*be_, cms_, *decoded.icc_profile)).first;
        return it->second->get();
    }
    std::shared_ptr<HipBackend> be_;
    EvalConfig config_;
    std::vector<CodecEntry> codecs_;
    Cms cms_;
    mutable std::map<std::vector<uint8_t>, std::unique_ptr<HipColorTable>> tables_;
};

// ---- crates/codec-iter: the SSIMULACRA2 plug point ---------------------------------------------------------
// Ssimulacra2Reference::{new, compare} (fast-ssim2; used at crates/codec-iter/src/eval.rs:138-149,83-89 and
// crates/codec-compare/src/brute_force_sweep.rs:197-201,256): the source image is uploaded once and its
// reference-side state stays on the device for the whole quality sweep.
class Ssimulacra2Reference {
public:
    Ssimulacra2Reference(std::shared_ptr<HipBackend> be, const std::vector<uint8_t> &rgb, size_t width, size_t height)
        : be_(std::move(be)), w_(width), h_(height)
    {
        const int rc = ce_ref_create(be_->ctx(), rgb.data(), rgb.size(), (uint32_t)width, (uint32_t)height, 0, &ref_);
        if (rc != CE_OK) throw Error(Error::Kind::MetricCalculation, "SSIM2 reference error: " + be_->last_error());
    }
    ~Ssimulacra2Reference() { ce_ref_destroy(ref_); }
    Ssimulacra2Reference(const Ssimulacra2Reference &) = delete;
    Ssimulacra2Reference &operator=(const Ssimulacra2Reference &) = delete;

    double compare(const std::vector<uint8_t> &distorted) const
    {
        ce_scores s{};
        const int rc = ce_ref_compare(ref_, distorted.data(), distorted.size(), CE_METRIC_SSIMULACRA2, CE_DEFAULT_INTENSITY_TARGET, &s);
        detail::check(*be_, rc, "SSIMULACRA2", w_, h_, distorted.size());
        return s.ssimulacra2;
    }
    // the sweep `for q in qualities { reference.compare(decoded[q]) }` (eval.rs:83-89) as one launch
    std::vector<double> compare_many(const std::vector<std::vector<uint8_t>> &distorted) const
    {
        std::vector<const uint8_t *> ptrs;
        std::vector<size_t> lens;
        for (const auto &d : distorted) {
            ptrs.push_back(d.data());
            lens.push_back(d.size());
        }
        std::vector<ce_scores> s(distorted.size());
        const int rc = ce_ref_compare_many(ref_, ptrs.data(), lens.data(), (uint32_t)distorted.size(), CE_METRIC_SSIMULACRA2,
                                           CE_DEFAULT_INTENSITY_TARGET, s.data());
        detail::check(*be_, rc, "SSIMULACRA2", w_, h_, 0);
        std::vector<double> out;
        for (size_t i = 0; i < s.size(); i++) {
            detail::check(*be_, s[i].status, "SSIMULACRA2", w_, h_, lens[i]);
            out.push_back(s[i].ssimulacra2);
        }
        return out;
    }

    // compute_heuristics of the resident source image (no second upload)
    ce_image_heuristics heuristics() const
    {
        ce_image_heuristics h{};
        detail::check(*be_, ce_ref_image_heuristics(ref_, &h), "image heuristics", w_, h_, 0);
        return h;
    }

private:
    std::shared_ptr<HipBackend> be_;
    ce_ref *ref_ = nullptr;
    size_t w_, h_;
};

// GpuSsim2 (crates/codec-iter/src/gpu.rs:21-134): `new(w, h)` fixes the shape, `compute(&mut self, ref, dis)`
// takes packed RGB8 from host memory and returns the score; one call in flight per object.
class GpuSsim2 {
public:
    GpuSsim2(uint32_t width, uint32_t height, int device = 0) : be_(std::make_shared<HipBackend>(device)), w_(width), h_(height) {}
    double compute(const std::vector<uint8_t> &reference, const std::vector<uint8_t> &distorted)
    {
        const size_t expected = (size_t)w_ * h_ * 3;
        if (reference.size() != expected || distorted.size() != expected)  // gpu.rs:84-94
            throw std::runtime_error("Image size mismatch: expected " + std::to_string(expected) + " bytes (" + std::to_string(w_) + "x" +
                                     std::to_string(h_) + "x3), got ref=" + std::to_string(reference.size()) +
                                     " dis=" + std::to_string(distorted.size()));
        double out = 0.0;
        const int rc = ce_calculate_ssimulacra2(be_->ctx(), reference.data(), reference.size(), distorted.data(), distorted.size(), w_, h_, &out);
        if (rc != CE_OK) throw std::runtime_error("SSIM2 HIP compute failed: " + be_->last_error());
        return out;
    }
    std::pair<uint32_t, uint32_t> dimensions() const { return {w_, h_}; }
    const std::shared_ptr<HipBackend> &backend() const { return be_; }

private:
    std::shared_ptr<HipBackend> be_;
    uint32_t w_, h_;
};

// Ssim2Backend (eval.rs:56-92).  The reference's enum has a Gpu and a Cpu arm; this library IS the device arm,
// so the mirror has that arm only (there is no CPU path in the product).  With a precomputed reference handle
// the source image is not uploaded again.
class Ssim2Backend {
public:
    explicit Ssim2Backend(std::unique_ptr<GpuSsim2> gpu) : gpu_(std::move(gpu)) {}
    double compare_with_precomputed(const std::vector<uint8_t> &source, const std::vector<uint8_t> &decoded,
                                    const Ssimulacra2Reference *reference, const std::string &image_name, unsigned quality)
    {
        try {
            return reference ? reference->compare(decoded) : gpu_->compute(source, decoded);
        } catch (const std::exception &e) {  // eval.rs:88
            throw std::runtime_error("SSIM2 error for " + image_name + " q" + std::to_string(quality) + ": " + e.what());
        }
    }
    GpuSsim2 &gpu() { return *gpu_; }

private:
    std::unique_ptr<GpuSsim2> gpu_;
};

// ---- src/eval/helpers.rs ---------------------------------------------------------------------------------
// evaluate_single, helpers.rs:105-173 (RGB8 images)
inline MetricResult evaluate_single(const HipBackend &be, const ImageData &reference, const ImageData &encoded, const MetricConfig &config)
{
    if (reference.width != encoded.width || reference.height != encoded.height)  // :111-116
        throw Error(Error::Kind::DimensionMismatch, "Dimension mismatch: expected (" + std::to_string(reference.width) + ", " +
                                                        std::to_string(reference.height) + "), got (" + std::to_string(encoded.width) +
                                                        ", " + std::to_string(encoded.height) + ")");
    const auto r = reference.to_rgb8_vec(), e = encoded.to_rgb8_vec();
    ce_scores s{};
    const int rc = ce_eval_pair(be.ctx(), r.data(), r.size(), e.data(), e.size(), (uint32_t)reference.width, (uint32_t)reference.height,
                                config.mask(), config.flags(), CE_DEFAULT_INTENSITY_TARGET, &s);
    detail::check(be, rc, "evaluate_single", reference.width, reference.height, e.size());
    return MetricResult::from_c(s);
}
// ---- deep input (include/ce_metrics.h: ce_batch_create_deep; no reference item - the reference rounds PixelData::Rgb16 to
// 8 bits with to_8bit before it measures) -------------------------------------------------------------------------------
// One pair of packed u16 RGB at its own precision: sample v of a side of depth d (8, 10, 12, 16) is the sRGB value
// v / (2^d - 1).  PSNR is reported for equal depths only.
inline MetricResult evaluate_pair_deep(const HipBackend &be, const std::vector<uint16_t> &reference, uint32_t ref_depth,
                                       const std::vector<uint16_t> &test, uint32_t test_depth, size_t width, size_t height,
                                       const MetricConfig &config)
{
    ce_scores s{};
    const int rc = ce_eval_pair_deep(be.ctx(), reference.data(), reference.size() * 2, ref_depth, test.data(), test.size() * 2, test_depth,
                                     (uint32_t)width, (uint32_t)height, config.mask(), config.flags(), CE_DEFAULT_INTENSITY_TARGET, &s);
    detail::check(be, rc, "evaluate_pair_deep", width, height, test.size());
    return MetricResult::from_c(s);
}
// A deep HBM-resident grid, filled with ce_batch_set_*_fmt(CE_PIXEL_RGB16 / CE_PIXEL_RGBA16) and run like any batch; the
// caller destroys it with ce_batch_destroy.
inline ce_batch *batch_deep(const HipBackend &be, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs,
                            uint32_t ref_depth, uint32_t test_depth)
{
    ce_batch *b = nullptr;
    const int rc = ce_batch_create_deep(be.ctx(), width, height, max_refs, max_pairs, ref_depth, test_depth, &b);
    detail::check(be, rc, "batch_deep", width, height, (size_t)width * height * 3);
    return b;
}
// ---- linear input (include/ce_metrics.h: ce_batch_create_linear) --------------------------------
// One pair of packed float RGB in linear light with BT.709 / sRGB primaries: 1.0 is the white an 8-bit 255 maps to, values
// below 0 and above 1 are scored.  PSNR is not reported.  intensity_target is Butteraugli's: nits at 1.0.
inline MetricResult evaluate_pair_linear(const HipBackend &be, const std::vector<float> &reference, const std::vector<float> &test,
                                         size_t width, size_t height, const MetricConfig &config,
                                         float intensity_target = CE_DEFAULT_INTENSITY_TARGET)
{
    ce_scores s{};
    const int rc = ce_eval_pair_linear(be.ctx(), reference.data(), reference.size() * 4, test.data(), test.size() * 4, (uint32_t)width,
                                       (uint32_t)height, config.mask(), config.flags(), intensity_target, &s);
    detail::check(be, rc, "evaluate_pair_linear", width, height, test.size());
    return MetricResult::from_c(s);
}
// The same pair at the size `condition` displays it (viewing::SimulationParams::displayed_size): both images resampled in
// linear light on the device (metrics::resample_linear), then scored; a condition that displays them as they are scores them
// as they are.  A resident grid takes the same route without a host copy: ce_batch_resample_pairs from one batch_linear into
// another of the displayed shape.
inline MetricResult evaluate_pair_linear_under(const HipBackend &be, const std::vector<float> &reference, const std::vector<float> &test,
                                               size_t width, size_t height, const viewing::ViewingCondition &condition,
                                               viewing::SimulationMode mode, const MetricConfig &config, int filter = CE_RESAMPLE_LANCZOS3,
                                               float intensity_target = CE_DEFAULT_INTENSITY_TARGET)
{
    const auto shown = condition.simulation_params((uint32_t)width, (uint32_t)height, mode).displayed_size((uint32_t)width, (uint32_t)height);
    if (shown == std::make_pair((uint32_t)width, (uint32_t)height)) return evaluate_pair_linear(be, reference, test, width, height, config, intensity_target);
    return evaluate_pair_linear(be, metrics::resample_linear(be, reference, (uint32_t)width, (uint32_t)height, shown.first, shown.second, filter),
                                metrics::resample_linear(be, test, (uint32_t)width, (uint32_t)height, shown.first, shown.second, filter), shown.first,
                                shown.second, config, intensity_target);
}
// A linear HBM-resident grid, filled with ce_batch_set_*_fmt(CE_PIXEL_RGB_F32) or metrics::batch_set_*_cicp and run like
// any batch; the caller destroys it with ce_batch_destroy.
inline ce_batch *batch_linear(const HipBackend &be, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t max_pairs)
{
    ce_batch *b = nullptr;
    const int rc = ce_batch_create_linear(be.ctx(), width, height, max_refs, max_pairs, &b);
    detail::check(be, rc, "batch_linear", width, height, (size_t)width * height * 3);
    return b;
}
// assert_quality, helpers.rs:212-255
inline void assert_quality(const HipBackend &be, const ImageData &reference, const ImageData &encoded,
                           std::optional<double> min_ssimulacra2, std::optional<double> max_dssim)
{
    MetricConfig cfg;
    cfg.dssim = max_dssim.has_value();
    cfg.ssimulacra2 = min_ssimulacra2.has_value();
    const MetricResult res = evaluate_single(be, reference, encoded, cfg);
    if (min_ssimulacra2 && res.ssimulacra2 && *res.ssimulacra2 < *min_ssimulacra2)
        throw Error(Error::Kind::QualityBelowThreshold, "SSIMULACRA2 quality below threshold: " + std::to_string(*res.ssimulacra2) +
                                                            " (threshold: " + std::to_string(*min_ssimulacra2) + ")");
    if (max_dssim && res.dssim && *res.dssim > *max_dssim)
        throw Error(Error::Kind::QualityBelowThreshold, "DSSIM quality below threshold: " + std::to_string(*res.dssim) +
                                                            " (threshold: " + std::to_string(*max_dssim) + ")");
}
// assert_perception_level, helpers.rs:291-321 (DSSIM only, ordinal compare)
inline void assert_perception_level(const HipBackend &be, const ImageData &reference, const ImageData &encoded, PerceptionLevel min_level)
{
    MetricConfig cfg;
    cfg.dssim = true;
    const MetricResult res = evaluate_single(be, reference, encoded, cfg);
    if (res.dssim && (uint8_t)perception_from_dssim(*res.dssim) > (uint8_t)min_level)
        throw Error(Error::Kind::QualityBelowThreshold, "PerceptionLevel (DSSIM " + std::to_string(*res.dssim) + ") below threshold");
}

}  // namespace eval
}  // namespace codec_eval
