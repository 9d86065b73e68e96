// Matrix/TRC ICC profiles applied on the device (include/ce_metrics.h: ce_batch_set_*_icc, ce_icc_to_*):
// a decoder's RGB code values -> linear light with BT.709 / sRGB primaries as packed f32 RGB (a linear slot: cicp_kernel.h's
// k_tagged with icc_pixel.h's icc_px), or -> sRGB code values as packed u8 or u16 RGB (an RGB8 slot, a deep side: icc_kernel.h's
// k_icc_encode around the same pixel).  One launch per image.  Per pixel: three gathers from the profile's host-built tone
// tables, an optional 3 x 3 in separately rounded f32 products and sums, the clamp of a linear image and, for integer slots,
// three branch-free searches of D steps in the host-built sRGB code thresholds.  No curve is evaluated here, and everything
// is compiled with -ffp-contract=off, so numpy reproduces it bit for bit (tests/icc_restatement.py).
//
// Streaming kernels of 3-8 bytes in and 3-12 bytes out per pixel; a thread owns four pixels, loaded and - into linear slots -
// stored as cicp.hip describes, into integer slots as three 4- or 8-byte stores where the slot's offset allows.  Tables and
// thresholds stay in global memory at every depth (vector L1 up to depth 12, L2 at 16).  No LDS, no scratch.
#include "ce_internal.h"

#include "icc_kernel.h"
#include "over_linear_kernel.h"

namespace {

// what a launch reports to the profiler: [slot kind: f32, u8, u16][format][with the matrix]
constexpr const char *kIccNames[3][4][2] = {
    {{"icc_lin_rgb8", "icc_lin_rgb8_m"}, {"icc_lin_rgba8", "icc_lin_rgba8_m"}, {"icc_lin_rgb16", "icc_lin_rgb16_m"}, {"icc_lin_rgba16", "icc_lin_rgba16_m"}},
    {{"icc_u8_rgb8", "icc_u8_rgb8_m"}, {"icc_u8_rgba8", "icc_u8_rgba8_m"}, {"icc_u8_rgb16", "icc_u8_rgb16_m"}, {"icc_u8_rgba16", "icc_u8_rgba16_m"}},
    {{"icc_u16_rgb8", "icc_u16_rgb8_m"}, {"icc_u16_rgba8", "icc_u16_rgba8_m"}, {"icc_u16_rgb16", "icc_u16_rgb16_m"}, {"icc_u16_rgba16", "icc_u16_rgba16_m"}}};

// kind: 0 a linear slot, 1 a u8 slot, 2 a u16 slot
template <int FMT, bool MATRIX>
void launch_one(ce_ctx *ctx, hipStream_t stream, const char *name, dim3 grid, const icc_args &a, int kind, void *d_dst, const float *d_thr, uint32_t top)
{
    const icc_px<MATRIX> px{a};
    if (kind == 0) CE_LAUNCH_ON(ctx, stream, name, (k_tagged<FMT, icc_px<MATRIX>>), grid, dim3(kCicpBlock), 0, px);
    else if (kind == 1) CE_LAUNCH_ON(ctx, stream, name, (k_icc_encode<FMT, false, icc_px<MATRIX>>), grid, dim3(kCicpBlock), 0, px, d_dst, d_thr, top);
    else CE_LAUNCH_ON(ctx, stream, name, (k_icc_encode<FMT, true, icc_px<MATRIX>>), grid, dim3(kCicpBlock), 0, px, d_dst, d_thr, top);
}

template <int FMT>
void launch_format(ce_ctx *ctx, hipStream_t stream, const char *const (&names)[2], dim3 grid, const icc_args &a, bool matrix, int kind, void *d_dst,
                   const float *d_thr, uint32_t top)
{
    if (matrix) launch_one<FMT, true>(ctx, stream, names[1], grid, a, kind, d_dst, d_thr, top);
    else launch_one<FMT, false>(ctx, stream, names[0], grid, a, kind, d_dst, d_thr, top);
}

// the pixel of a linear slot blended over solid backgrounds (over_linear_kernel.h): [RGBA16][with the matrix]
constexpr const char *kIccOverNames[2][2] = {{"icc_over_rgba8", "icc_over_rgba8_m"}, {"icc_over_rgba16", "icc_over_rgba16_m"}};

template <int FMT>
void launch_over(ce_ctx *ctx, hipStream_t stream, const char *const (&names)[2], dim3 grid, const icc_args &a, bool matrix, const over_args &o)
{
    if (matrix) CE_LAUNCH_ON(ctx, stream, names[1], (k_tagged_over<FMT, icc_px<true>>), grid, dim3(kCicpBlock), 0, icc_px<true>{a}, o);
    else CE_LAUNCH_ON(ctx, stream, names[0], (k_tagged_over<FMT, icc_px<false>>), grid, dim3(kCicpBlock), 0, icc_px<false>{a}, o);
}

}  // namespace

int ce_launch_icc(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                  const ce_over_plan *ov)
{
    if (n_pixels == 0) return CE_OK;
    if (ov && (px.depth_out != 0 || !ov->d_atab || ov->n_bg == 0 || ov->n_bg > CE_MAX_BACKGROUNDS ||
               (format != CE_PIXEL_RGBA8 && format != CE_PIXEL_RGBA16))) {
        ctx->err = "ICC composite: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    if (px.lut) return ce_launch_icc_lut(ctx, stream, format, d_src, d_dst, n_pixels, px, ov);
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    const bool integer = px.depth_out != 0;
    if (blocks > 0x7fffffffu || !px.d_tables || !d_src || !d_dst || (integer && !px.d_thr)) {
        ctx->err = "ICC ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    icc_args a{};
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    a.c.dst = integer ? nullptr : static_cast<float *>(d_dst);
    ce_fill_icc_args(a, px);
    const int kind = !integer ? 0 : px.out16 ? 2 : 1;
    const uint32_t top = integer ? 1u << (px.depth_out - 1) : 0u;
    const dim3 grid((uint32_t)blocks);
    if (ov) {
        over_args o{};
        ce_fill_over_args(o, *ov);
        if (format == CE_PIXEL_RGBA16) launch_over<CE_PIXEL_RGBA16>(ctx, stream, kIccOverNames[1], grid, a, px.has_matrix, o);
        else launch_over<CE_PIXEL_RGBA8>(ctx, stream, kIccOverNames[0], grid, a, px.has_matrix, o);
        CE_HIP(ctx, hipGetLastError());
        return CE_OK;
    }
    switch (format) {
        case CE_PIXEL_RGB8: launch_format<CE_PIXEL_RGB8>(ctx, stream, kIccNames[kind][0], grid, a, px.has_matrix, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGBA8: launch_format<CE_PIXEL_RGBA8>(ctx, stream, kIccNames[kind][1], grid, a, px.has_matrix, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGB16: launch_format<CE_PIXEL_RGB16>(ctx, stream, kIccNames[kind][2], grid, a, px.has_matrix, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGBA16: launch_format<CE_PIXEL_RGBA16>(ctx, stream, kIccNames[kind][3], grid, a, px.has_matrix, kind, d_dst, px.d_thr, top); break;
        default: ctx->err = "ICC ingest: format must be RGB8, RGBA8, RGB16 or RGBA16"; return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
