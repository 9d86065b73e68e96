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
// The launcher's body is icc_launch.h's, shared with icc_lut.hip; this file adds the pixel (icc_px<with the matrix>) and its fill.
#include "ce_internal.h"

#include "icc_launch.h"

int ce_launch_icc(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
                  const ce_over_plan *ov)
{
    if (n_pixels == 0) return CE_OK;
    if (ov && (px.depth_out != 0 || !ov->d_atab || ov->n_bg == 0 || ov->n_bg > CE_MAX_BACKGROUNDS || !packed_has_alpha(format))) {
        ctx->err = "ICC composite: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    if (px.lut) return ce_launch_icc_lut(ctx, stream, format, d_src, d_dst, n_pixels, px, ov);
    return icc_launch<icc_px, icc_args>(ctx, stream, format, d_src, d_dst, n_pixels, px, ov, px.has_matrix, "icc", px.has_matrix ? "_m" : "",
                                        [&](icc_args &a) { ce_fill_icc_args(a, px); });
}
