// Ingest of tagged code values on the device (include/ce_metrics.h: ce_batch_set_*_cicp, ce_cicp_to_linear, ce_batch_set_*_hlg,
// ce_hlg_to_linear; DESIGN.md sections 15 and 18): a decoder's RGB code values -> linear light with BT.709 / sRGB primaries, as
// packed f32 RGB in a slot of a linear batch.  One launch per image, one frame (cicp_kernel.h: k_tagged) and two pixels.
// CICP, H.273 colour primaries and transfer characteristics: sample -> host-built transfer table (the curve is never
// evaluated here) -> optional 3 x 3 primaries matrix in separately rounded f32 products and sums -> NaN / range clamp of a
// linear image.  HLG, BT.2100: sample -> host-built inverse-OETF table -> scene luminance in f64 -> Ys^(gamma - 1) through
// hlg_pow, a fixed sequence of correctly rounded f64 operations (hlg_pixel.h) -> one f32 scale to display light -> the same
// matrix and clamp.  Everything is compiled with -ffp-contract=off, so numpy reproduces both bit for bit
// (tests/cicp_restatement.py, tests/hlg_restatement.py).  The same file holds the CE_PIXEL_RGB_F32 upload's clamp pass.
//
// A streaming kernel of 3-8 bytes in and 12 bytes out per pixel; on top of the gather and the stores an HLG pixel costs
// about 70 f64 operations, two of them divisions.  A thread owns four pixels: aligned dword / 8- / 16-byte
// loads from the staging image and three 16-byte stores where the slot is 16-byte aligned (slot k of the slab starts at
// k * w * h * 12 bytes, so every slot of an image with w * h a multiple of 4 and slot 0 of any image), twelve 4-byte stores
// otherwise - a branch the whole launch takes alike.  The table stays in global memory at every depth: the 1, 4
// and 16 KB tables live in the vector L1 after the first touch, the 256 KB table of depth 16 in L2 (the gather section 11
// measured as small beside the front ends' arithmetic), and one code path serves all four.  No LDS, no scratch.
#include "ce_internal.h"

#include "cicp_kernel.h"
#include "hlg_pixel.h"
#include "over_linear_kernel.h"

int ce_launch_linear_sanitise(ce_ctx *ctx, hipStream_t stream, const float *d_src, float *d_dst, size_t n_samples)
{
    if (n_samples == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_samples / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu) {
        ctx->err = "linear upload: image too large";
        return CE_ERR_INVALID_ARG;
    }
    CE_LAUNCH_ON(ctx, stream, "ingest_linear_f32", k_linear_sanitise, dim3((uint32_t)blocks), dim3(kCicpBlock), 0, d_src, d_dst, n_samples);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

namespace {

// what a launch reports to the profiler: [HLG][format][with the primaries matrix]
constexpr const char *kTaggedNames[2][4][2] = {
    {{"cicp_rgb8", "cicp_rgb8_m"}, {"cicp_rgba8", "cicp_rgba8_m"}, {"cicp_rgb16", "cicp_rgb16_m"}, {"cicp_rgba16", "cicp_rgba16_m"}},
    {{"hlg_rgb8", "hlg_rgb8_m"}, {"hlg_rgba8", "hlg_rgba8_m"}, {"hlg_rgb16", "hlg_rgb16_m"}, {"hlg_rgba16", "hlg_rgba16_m"}}};

template <int FMT, template <bool> class Px, class Args>
void launch_format(ce_ctx *ctx, hipStream_t stream, const char *const (&names)[2], dim3 grid, const Args &a, bool matrix)
{
    if (matrix) CE_LAUNCH_ON(ctx, stream, names[1], (k_tagged<FMT, Px<true>>), grid, dim3(kCicpBlock), 0, Px<true>{a});
    else CE_LAUNCH_ON(ctx, stream, names[0], (k_tagged<FMT, Px<false>>), grid, dim3(kCicpBlock), 0, Px<false>{a});
}

// false: not one of the four formats
template <template <bool> class Px, class Args>
bool launch_pixel(ce_ctx *ctx, hipStream_t stream, int format, const char *const (&names)[4][2], dim3 grid, const Args &a, bool matrix)
{
    switch (format) {
        case CE_PIXEL_RGB8: launch_format<CE_PIXEL_RGB8, Px>(ctx, stream, names[0], grid, a, matrix); return true;
        case CE_PIXEL_RGBA8: launch_format<CE_PIXEL_RGBA8, Px>(ctx, stream, names[1], grid, a, matrix); return true;
        case CE_PIXEL_RGB16: launch_format<CE_PIXEL_RGB16, Px>(ctx, stream, names[2], grid, a, matrix); return true;
        case CE_PIXEL_RGBA16: launch_format<CE_PIXEL_RGBA16, Px>(ctx, stream, names[3], grid, a, matrix); return true;
        default: return false;
    }
}

}  // namespace

int ce_launch_tagged(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const ce_linear_pixel &px)
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu || !px.d_table) {
        ctx->err = px.hlg ? "HLG ingest: bad launch" : "CICP ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    hlg_args a{};  // the CICP pixel takes its `c` alone
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    ce_fill_pixel_args(a, d_dst, px);
    const dim3 grid((uint32_t)blocks);
    // the one place that knows which pixel a plan means
    if (!(px.hlg ? launch_pixel<hlg_px>(ctx, stream, format, kTaggedNames[1], grid, a, px.has_matrix)
                 : launch_pixel<cicp_px>(ctx, stream, format, kTaggedNames[0], grid, a.c, px.has_matrix))) {
        ctx->err = std::string(px.hlg ? "HLG" : "CICP") + " ingest: format must be RGB8, RGBA8, RGB16 or RGBA16";
        return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

// ---- the same pixels blended over solid backgrounds in linear light (over_linear_kernel.h) ----------------

namespace {

// [HLG][RGBA16][with the primaries matrix]
constexpr const char *kOverNames[2][2][2] = {{{"cicp_over_rgba8", "cicp_over_rgba8_m"}, {"cicp_over_rgba16", "cicp_over_rgba16_m"}},
                                             {{"hlg_over_rgba8", "hlg_over_rgba8_m"}, {"hlg_over_rgba16", "hlg_over_rgba16_m"}}};

template <int FMT, template <bool> class Px, class Args>
void launch_over_format(ce_ctx *ctx, hipStream_t stream, const char *const (&names)[2], dim3 grid, const Args &a, bool matrix, const over_args &o)
{
    if (matrix) CE_LAUNCH_ON(ctx, stream, names[1], (k_tagged_over<FMT, Px<true>>), grid, dim3(kCicpBlock), 0, Px<true>{a}, o);
    else CE_LAUNCH_ON(ctx, stream, names[0], (k_tagged_over<FMT, Px<false>>), grid, dim3(kCicpBlock), 0, Px<false>{a}, o);
}

template <template <bool> class Px, class Args>
void launch_over_pixel(ce_ctx *ctx, hipStream_t stream, bool wide, const char *const (&names)[2][2], dim3 grid, const Args &a, bool matrix,
                       const over_args &o)
{
    if (wide) launch_over_format<CE_PIXEL_RGBA16, Px>(ctx, stream, names[1], grid, a, matrix, o);
    else launch_over_format<CE_PIXEL_RGBA8, Px>(ctx, stream, names[0], grid, a, matrix, o);
}

}  // namespace

int ce_launch_tagged_over(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const ce_linear_pixel &px,
                          const ce_over_plan &ov)
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu || !px.d_table || !ov.d_atab || ov.n_bg == 0 || ov.n_bg > CE_MAX_BACKGROUNDS ||
        (format != CE_PIXEL_RGBA8 && format != CE_PIXEL_RGBA16)) {
        ctx->err = px.hlg ? "HLG composite: bad launch" : "CICP composite: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    hlg_args a{};  // the CICP pixel takes its `c` alone
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    ce_fill_pixel_args(a, d_dst, px);
    over_args o{};
    ce_fill_over_args(o, ov);
    const dim3 grid((uint32_t)blocks);
    if (px.hlg) launch_over_pixel<hlg_px>(ctx, stream, format == CE_PIXEL_RGBA16, kOverNames[1], grid, a, px.has_matrix, o);
    else launch_over_pixel<cicp_px>(ctx, stream, format == CE_PIXEL_RGBA16, kOverNames[0], grid, a.c, px.has_matrix, o);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

int ce_launch_linear_over(ce_ctx *ctx, hipStream_t stream, const float *d_src, float *d_dst, size_t n_pixels, bool premultiplied,
                          const ce_over_plan &ov)
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu || ov.n_bg == 0 || ov.n_bg > CE_MAX_BACKGROUNDS) {
        ctx->err = "linear composite: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    over_args o{};
    ce_fill_over_args(o, ov);
    const dim3 grid((uint32_t)blocks);
    if (premultiplied) CE_LAUNCH_ON(ctx, stream, "linear_over_premul", k_linear_over<true>, grid, dim3(kCicpBlock), 0, d_src, d_dst, n_pixels, o);
    else CE_LAUNCH_ON(ctx, stream, "linear_over", k_linear_over<false>, grid, dim3(kCicpBlock), 0, d_src, d_dst, n_pixels, o);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
