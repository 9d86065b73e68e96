// LUT-based ICC profiles applied on the device (include/ce_metrics.h: ce_icc_lut_create): the two frames
// of icc.hip - cicp_kernel.h's k_tagged for a linear slot, icc_kernel.h's k_icc_encode for a u8 or u16 slot - around
// icc_lut_pixel.h's pixel.  One launch per image.  Per pixel: three gathers from the host-built input tables, four (tetrahedral)
// or eight (trilinear) 16-byte loads of CLUT nodes, up to six post-CLUT curves - a sampled one is two gathers and a lerp, a
// power one about 80 f64 operations - the 3 x 4 matrix, the PCS decode, the 3 x 3 to sRGB primaries and the clamp; for integer
// slots the threshold search on top.  Which stages run is the same for every pixel of a launch.  Compiled with
// -ffp-contract=off, so numpy reproduces it bit for bit (tests/icc_lut_restatement.py).
//
// A 33^3 CLUT is 575 KB and stays in L2; neighbouring pixels of an image mostly share a cell, so the node loads of a wave hit
// few lines.  No LDS, no scratch.
#include "ce_internal.h"

#include "icc_kernel.h"
#include "icc_lut_pixel.h"
#include "over_linear_kernel.h"

namespace {

// what a launch reports to the profiler: [interpolation][slot kind: f32, u8, u16][format]
constexpr const char *kIccLutNames[2][3][4] = {
    {{"icc_lut_tri_lin_rgb8", "icc_lut_tri_lin_rgba8", "icc_lut_tri_lin_rgb16", "icc_lut_tri_lin_rgba16"},
     {"icc_lut_tri_u8_rgb8", "icc_lut_tri_u8_rgba8", "icc_lut_tri_u8_rgb16", "icc_lut_tri_u8_rgba16"},
     {"icc_lut_tri_u16_rgb8", "icc_lut_tri_u16_rgba8", "icc_lut_tri_u16_rgb16", "icc_lut_tri_u16_rgba16"}},
    {{"icc_lut_tet_lin_rgb8", "icc_lut_tet_lin_rgba8", "icc_lut_tet_lin_rgb16", "icc_lut_tet_lin_rgba16"},
     {"icc_lut_tet_u8_rgb8", "icc_lut_tet_u8_rgba8", "icc_lut_tet_u8_rgb16", "icc_lut_tet_u8_rgba16"},
     {"icc_lut_tet_u16_rgb8", "icc_lut_tet_u16_rgba8", "icc_lut_tet_u16_rgb16", "icc_lut_tet_u16_rgba16"}}};

// kind: 0 a linear slot, 1 a u8 slot, 2 a u16 slot
template <int FMT, bool TETRA>
void launch_one(ce_ctx *ctx, hipStream_t stream, const char *name, dim3 grid, const icc_lut_args &a, int kind, void *d_dst, const float *d_thr, uint32_t top)
{
    const icc_lut_px<TETRA> px{a};
    if (kind == 0) CE_LAUNCH_ON(ctx, stream, name, (k_tagged<FMT, icc_lut_px<TETRA>>), grid, dim3(kCicpBlock), 0, px);
    else if (kind == 1) CE_LAUNCH_ON(ctx, stream, name, (k_icc_encode<FMT, false, icc_lut_px<TETRA>>), grid, dim3(kCicpBlock), 0, px, d_dst, d_thr, top);
    else CE_LAUNCH_ON(ctx, stream, name, (k_icc_encode<FMT, true, icc_lut_px<TETRA>>), grid, dim3(kCicpBlock), 0, px, d_dst, d_thr, top);
}

template <int FMT>
void launch_format(ce_ctx *ctx, hipStream_t stream, int f, dim3 grid, const icc_lut_args &a, bool tetra, int kind, void *d_dst, const float *d_thr,
                   uint32_t top)
{
    if (tetra) launch_one<FMT, true>(ctx, stream, kIccLutNames[1][kind][f], grid, a, kind, d_dst, d_thr, top);
    else launch_one<FMT, false>(ctx, stream, kIccLutNames[0][kind][f], grid, a, kind, d_dst, d_thr, top);
}

// the pixel of a linear slot blended over solid backgrounds (over_linear_kernel.h): [interpolation][RGBA16]
constexpr const char *kIccLutOverNames[2][2] = {{"icc_lut_tri_over_rgba8", "icc_lut_tri_over_rgba16"}, {"icc_lut_tet_over_rgba8", "icc_lut_tet_over_rgba16"}};

template <int FMT>
void launch_over(ce_ctx *ctx, hipStream_t stream, int f, dim3 grid, const icc_lut_args &a, bool tetra, const over_args &o)
{
    if (tetra) CE_LAUNCH_ON(ctx, stream, kIccLutOverNames[1][f], (k_tagged_over<FMT, icc_lut_px<true>>), grid, dim3(kCicpBlock), 0, icc_lut_px<true>{a}, o);
    else CE_LAUNCH_ON(ctx, stream, kIccLutOverNames[0][f], (k_tagged_over<FMT, icc_lut_px<false>>), grid, dim3(kCicpBlock), 0, icc_lut_px<false>{a}, o);
}

}  // namespace

int ce_launch_icc_lut(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                      const ce_over_plan *ov)
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    const bool integer = px.depth_out != 0;
    const ce_icc_lut *lut = px.lut;
    if (blocks > 0x7fffffffu || !lut || !px.d_tables || !d_src || !d_dst || (integer && !px.d_thr)) {
        ctx->err = "ICC ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    icc_lut_args a{};
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    a.c.dst = integer ? nullptr : static_cast<float *>(d_dst);
    ce_fill_icc_lut_args(a, px);
    const int kind = !integer ? 0 : px.out16 ? 2 : 1;
    const uint32_t top = integer ? 1u << (px.depth_out - 1) : 0u;
    const dim3 grid((uint32_t)blocks);
    if (ov) {  // ce_launch_icc has checked the plan, the format and the slot kind
        over_args o{};
        ce_fill_over_args(o, *ov);
        if (format == CE_PIXEL_RGBA16) launch_over<CE_PIXEL_RGBA16>(ctx, stream, 1, grid, a, lut->tetra, o);
        else launch_over<CE_PIXEL_RGBA8>(ctx, stream, 0, grid, a, lut->tetra, o);
        CE_HIP(ctx, hipGetLastError());
        return CE_OK;
    }
    switch (format) {
        case CE_PIXEL_RGB8: launch_format<CE_PIXEL_RGB8>(ctx, stream, 0, grid, a, lut->tetra, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGBA8: launch_format<CE_PIXEL_RGBA8>(ctx, stream, 1, grid, a, lut->tetra, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGB16: launch_format<CE_PIXEL_RGB16>(ctx, stream, 2, grid, a, lut->tetra, kind, d_dst, px.d_thr, top); break;
        case CE_PIXEL_RGBA16: launch_format<CE_PIXEL_RGBA16>(ctx, stream, 3, grid, a, lut->tetra, kind, d_dst, px.d_thr, top); break;
        default: ctx->err = "ICC ingest: format must be RGB8, RGBA8, RGB16 or RGBA16"; return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
