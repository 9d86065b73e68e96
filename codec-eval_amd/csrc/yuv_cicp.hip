// Y'CbCr planes with a CICP or an HLG description straight into a slot of a linear batch (include/ce_metrics.h:
// ce_batch_set_*_yuv_cicp, ce_yuv_to_linear, ce_batch_set_*_yuv_hlg, ce_yuv_hlg_to_linear; DESIGN.md sections 16 and 18): what
// yuv.hip and cicp.hip do behind each other, in one launch per image and without the integer RGB image between them.  The
// definition is the composition of theirs and adds no arithmetic: a thread runs yuv_kernel.h's block (8 x 2 pixels: clamped
// loads, integer upsampling, int64 matrix, clamp to 2^depth - 1 of the description) and hands each pixel to the one cicp.hip
// would run: cicp_pixel.h's cicp_px (table gather from global memory, separately rounded f32 3 x 3 for primaries other than 1,
// clamp of a linear image) or hlg_pixel.h's hlg_px (-ffp-contract=off).  One frame, yuv_cicp_kernel.h's k_yuv_tagged.
//
// 1.5 - 6 bytes in and 12 bytes out per pixel.  A row of a thread's block is 24 floats, 96 bytes, at byte
// (slot * w * h + y * w + x0) * 12 of the slab: a multiple of 4 whose residue mod 16 changes with the slot, with y * w mod 4
// and with the image's size, so store24 picks 16-, 8- and 4-byte stores per row from the address (a wave's rows agree
// except where it wraps to the next row pair).  A cropped group stores sample by sample.  No LDS, no scratch.
#include "ce_internal.h"

#include "tagged_pick.h"
#include "yuv_cicp_kernel.h"
#include "yuv_ladder.h"

int ce_launch_yuv_tagged(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, float *d_dst, const ce_linear_pixel &px)
{
    if (w == 0 || h == 0) return CE_OK;
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    if (blocks > 0x7fffffffu || !px.d_table) {
        ctx->err = px.hlg ? "Y'CbCr HLG ingest: bad launch" : "Y'CbCr CICP ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    yuv_args y{};
    ce_fill_yuv_args(y, src, w, h, (int64_t)px.maxv);  // src.k was built for this output depth (yuv_check with depth_out = the description's depth)
    const dim3 grid((uint32_t)blocks);
    // the profile names follow yuv.hip's: subsampling, input sample size, then _lin or _hlg, and _m with the primaries matrix
    tagged_pick(px, nullptr, 0, d_dst, [&](const auto &pixel, const char *, const char *m) {
        using P = std::decay_t<decltype(pixel)>;
        char suffix[8];
        std::snprintf(suffix, sizeof suffix, "%s%s", px.hlg ? "_hlg" : "_lin", m);
        yuv_ladder(src.depth == 8, src.subsampling, src.layout == CE_YUV_SEMIPLANAR, [&](auto bps, auto sub, auto semi) {
            constexpr int BPS = decltype(bps)::value, SUB = decltype(sub)::value;
            constexpr bool SEMI = decltype(semi)::value;
            CE_LAUNCH_ON(ctx, stream, yuv_profile_name(SUB, BPS, suffix).s, (k_yuv_tagged<BPS, SUB, SEMI, P>), grid, dim3(64), 0, yuv_px_args<P>{y, pixel});
        });
    });
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
