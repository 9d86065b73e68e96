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
// The launcher's body is icc_launch.h's, shared with icc.hip; this file adds the pixel (icc_lut_px<tetrahedral>) and its fill.
#include "ce_internal.h"

#include "icc_launch.h"
#include "icc_lut_pixel.h"

int ce_launch_icc_lut(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                      const ce_over_plan *ov)
{
    if (n_pixels == 0) return CE_OK;
    if (!px.lut) {
        ctx->err = "ICC ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    const bool tetra = px.lut->tetra;
    return icc_launch<icc_lut_px, icc_lut_args>(ctx, stream, format, d_src, d_dst, n_pixels, px, ov, tetra, tetra ? "icc_lut_tet" : "icc_lut_tri", "",
                                                [&](icc_lut_args &a) { ce_fill_icc_lut_args(a, px); });
}
