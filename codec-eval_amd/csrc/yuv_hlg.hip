// Y'CbCr planes in BT.2100 HLG straight into a slot of a linear batch (include/ce_metrics.h: ce_batch_set_*_yuv_hlg,
// ce_yuv_hlg_to_linear): what yuv.hip and hlg.hip do behind each other, in one launch per image and
// without the integer RGB image between them.  The definition is the composition of theirs and adds no arithmetic: a thread
// runs yuv_kernel.h's block (8 x 2 pixels: clamped loads, integer upsampling, int64 matrix, clamp to 2^depth - 1 of the HLG
// description) and hands each pixel to hlg_pixel.h's hlg_pixel (-ffp-contract=off).  The frame - grid, store24's choice of
// store widths per row, the cropped group, the odd height - is yuv_cicp.hip's.  No LDS, no scratch.
#include "ce_internal.h"

#include "yuv_hlg_kernel.h"

namespace {

template <int BPS, int SUB>
void launch_layout(ce_ctx *ctx, hipStream_t stream, const char *name, const char *name_m, bool semi, bool matrix, dim3 grid, const yuv_hlg_args &a)
{
    if (semi && SUB != CE_YUV_400) {
        if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_yuv_hlg<BPS, SUB, true, true>), grid, dim3(64), 0, a);
        else CE_LAUNCH_ON(ctx, stream, name, (k_yuv_hlg<BPS, SUB, true, false>), grid, dim3(64), 0, a);
    } else {
        if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_yuv_hlg<BPS, SUB, false, true>), grid, dim3(64), 0, a);
        else CE_LAUNCH_ON(ctx, stream, name, (k_yuv_hlg<BPS, SUB, false, false>), grid, dim3(64), 0, a);
    }
}

template <int BPS>
void launch_sub(ce_ctx *ctx, hipStream_t stream, int sub, bool semi, bool matrix, dim3 grid, const yuv_hlg_args &a)
{
    // the profile names follow yuv_cicp.hip's: input sample size, subsampling, HLG output, _m with the primaries matrix
    switch (sub) {
        case CE_YUV_444: launch_layout<BPS, CE_YUV_444>(ctx, stream, BPS == 1 ? "yuv444_8_hlg" : "yuv444_16_hlg", BPS == 1 ? "yuv444_8_hlg_m" : "yuv444_16_hlg_m", semi, matrix, grid, a); break;
        case CE_YUV_422: launch_layout<BPS, CE_YUV_422>(ctx, stream, BPS == 1 ? "yuv422_8_hlg" : "yuv422_16_hlg", BPS == 1 ? "yuv422_8_hlg_m" : "yuv422_16_hlg_m", semi, matrix, grid, a); break;
        case CE_YUV_420: launch_layout<BPS, CE_YUV_420>(ctx, stream, BPS == 1 ? "yuv420_8_hlg" : "yuv420_16_hlg", BPS == 1 ? "yuv420_8_hlg_m" : "yuv420_16_hlg_m", semi, matrix, grid, a); break;
        default: launch_layout<BPS, CE_YUV_400>(ctx, stream, BPS == 1 ? "yuv400_8_hlg" : "yuv400_16_hlg", BPS == 1 ? "yuv400_8_hlg_m" : "yuv400_16_hlg_m", semi, matrix, grid, a); break;
    }
}

}  // namespace

int ce_launch_yuv_hlg(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, float *d_dst, const float *d_table,
                      uint32_t maxv, const float *matrix, const double params[5])
{
    if (w == 0 || h == 0) return CE_OK;
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    if (blocks > 0x7fffffffu || !d_table) {
        ctx->err = "Y'CbCr HLG ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    yuv_hlg_args a{};
    ce_fill_yuv_args(a.y, src, w, h, (int64_t)maxv);  // src.k was built for this output depth (yuv_check with depth_out = the HLG description's depth)
    ce_fill_cicp_args(a.h.c, d_dst, d_table, maxv, matrix);
    a.h.kr = params[0], a.h.kg = params[1], a.h.kb = params[2], a.h.gm1 = params[3], a.h.a = params[4];
    const dim3 grid((uint32_t)blocks);
    const bool semi = src.layout == CE_YUV_SEMIPLANAR;
    if (src.depth == 8) launch_sub<1>(ctx, stream, src.subsampling, semi, matrix != nullptr, grid, a);
    else launch_sub<2>(ctx, stream, src.subsampling, semi, matrix != nullptr, grid, a);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
