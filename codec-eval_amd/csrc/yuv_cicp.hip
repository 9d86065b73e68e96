// Y'CbCr planes with a CICP description straight into a slot of a linear batch (include/ce_metrics.h:
// ce_batch_set_*_yuv_cicp, ce_yuv_to_linear): what yuv.hip and cicp.hip do behind each other, in one
// launch per image and without the integer RGB image between them.  The definition is the composition of theirs and adds no
// arithmetic: a thread runs yuv_kernel.h's block (8 x 2 pixels: clamped loads, integer upsampling, int64 matrix, clamp to
// 2^depth - 1 of the colour description) and hands each pixel to cicp_pixel.h's cicp_pixel (table gather from global memory,
// separately rounded f32 3 x 3 for primaries other than 1, clamp of a linear image; -ffp-contract=off).
//
// 1.5 - 6 bytes in and 12 bytes out per pixel.  A row of a thread's block is 24 floats, 96 bytes, at byte
// (slot * w * h + y * w + x0) * 12 of the slab: a multiple of 4 whose residue mod 16 changes with the slot, with y * w mod 4
// and with the image's size, so store24 picks 16-, 8- and 4-byte stores per row from the address (a wave's rows agree
// except where it wraps to the next row pair).  A cropped group stores sample by sample.  No LDS, no scratch.
#include "ce_internal.h"

#include "yuv_cicp_kernel.h"

namespace {

template <int BPS, int SUB>
void launch_layout(ce_ctx *ctx, hipStream_t stream, const char *name, const char *name_m, bool semi, bool matrix, dim3 grid, const yuv_cicp_args &a)
{
    if (semi && SUB != CE_YUV_400) {
        if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_yuv_cicp<BPS, SUB, true, true>), grid, dim3(64), 0, a);
        else CE_LAUNCH_ON(ctx, stream, name, (k_yuv_cicp<BPS, SUB, true, false>), grid, dim3(64), 0, a);
    } else {
        if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_yuv_cicp<BPS, SUB, false, true>), grid, dim3(64), 0, a);
        else CE_LAUNCH_ON(ctx, stream, name, (k_yuv_cicp<BPS, SUB, false, false>), grid, dim3(64), 0, a);
    }
}

template <int BPS>
void launch_sub(ce_ctx *ctx, hipStream_t stream, int sub, bool semi, bool matrix, dim3 grid, const yuv_cicp_args &a)
{
    // the profile names follow yuv.hip's: input sample size, subsampling, linear output, _m with the primaries matrix
    switch (sub) {
        case CE_YUV_444: launch_layout<BPS, CE_YUV_444>(ctx, stream, BPS == 1 ? "yuv444_8_lin" : "yuv444_16_lin", BPS == 1 ? "yuv444_8_lin_m" : "yuv444_16_lin_m", semi, matrix, grid, a); break;
        case CE_YUV_422: launch_layout<BPS, CE_YUV_422>(ctx, stream, BPS == 1 ? "yuv422_8_lin" : "yuv422_16_lin", BPS == 1 ? "yuv422_8_lin_m" : "yuv422_16_lin_m", semi, matrix, grid, a); break;
        case CE_YUV_420: launch_layout<BPS, CE_YUV_420>(ctx, stream, BPS == 1 ? "yuv420_8_lin" : "yuv420_16_lin", BPS == 1 ? "yuv420_8_lin_m" : "yuv420_16_lin_m", semi, matrix, grid, a); break;
        default: launch_layout<BPS, CE_YUV_400>(ctx, stream, BPS == 1 ? "yuv400_8_lin" : "yuv400_16_lin", BPS == 1 ? "yuv400_8_lin_m" : "yuv400_16_lin_m", semi, matrix, grid, a); break;
    }
}

}  // namespace

int ce_launch_yuv_cicp(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, float *d_dst, const float *d_table,
                       uint32_t maxv, const float *matrix)
{
    if (w == 0 || h == 0) return CE_OK;
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    if (blocks > 0x7fffffffu || !d_table) {
        ctx->err = "Y'CbCr CICP ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    yuv_cicp_args a{};
    ce_fill_yuv_args(a.y, src, w, h, (int64_t)maxv);  // src.k was built for this output depth (yuv_check with depth_out = the colour description's depth)
    ce_fill_cicp_args(a.c, d_dst, d_table, maxv, matrix);
    const dim3 grid((uint32_t)blocks);
    const bool semi = src.layout == CE_YUV_SEMIPLANAR;
    if (src.depth == 8) launch_sub<1>(ctx, stream, src.subsampling, semi, matrix != nullptr, grid, a);
    else launch_sub<2>(ctx, stream, src.subsampling, semi, matrix != nullptr, grid, a);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
