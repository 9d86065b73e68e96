// Planar Y'CbCr ingest on the device (include/ce_metrics.h: ce_batch_set_*_yuv, ce_yuv_to_rgb*): a
// decoder's planes -> chroma upsampling -> colour matrix -> the packed RGB slot of a resident batch, one launch per image,
// all in integers.  The definition (libjpeg-turbo's h2v2 / h2v1 "fancy" upsampling and jdcolor.c's fixed point, with the
// coefficients generalised to other matrices, ranges and depths) is stated in the header.
//
// A thread owns 8 x 2 output pixels: both rows of one chroma row pair, four chroma columns.  It reads its 8 luma samples
// of each row as one 8- or 16-byte load, so a wave's loads of a luma row are contiguous, and the chroma samples it needs
// (4:2:0 / 4:2:2: four columns and one neighbour on each side, of the row above, its own and the one below) one by one at
// CLAMPED indices: the clamp is the filter's edge rule (c[max(r - 1, 0)], c[min(i + 1, cw - 1)]) and keeps every address
// inside the plane for the groups the crop to an odd width or height cuts, so there is no branch around a load.  Neighbours
// are shared with the adjacent threads through L1 / L2; no LDS.  CE_CHROMA_NEAREST is the same arithmetic with every
// neighbour replaced by the sample itself ((3 * 4c + 4c + 8) >> 4 = c), chosen by selects.  Semiplanar CbCr is read as
// one packed pair per sample.  A row of a thread's block is 24 bytes (u8) or 48 bytes (u16) of output: stored as 8- or
// 16-byte words where the address allows (slot k of an RGB8 slab starts at k * w * h * 3 bytes and a row at y * w * 3, so
// the alignment varies with both), as dwords where only that holds, sample by sample otherwise and in a cropped group.
#include "ce_internal.h"

#include "yuv_kernel.h"

namespace {

template <int BPS, bool OUT16, int SUB>
void launch_layout(ce_ctx *ctx, hipStream_t stream, const char *name, bool semi, dim3 grid, const yuv_args &a, uint8_t *dst)
{
    if (semi && SUB != CE_YUV_400) CE_LAUNCH_ON(ctx, stream, name, (k_yuv<BPS, OUT16, SUB, true>), grid, dim3(64), 0, a, dst);
    else CE_LAUNCH_ON(ctx, stream, name, (k_yuv<BPS, OUT16, SUB, false>), grid, dim3(64), 0, a, dst);
}

template <int BPS, bool OUT16>
void launch_sub(ce_ctx *ctx, hipStream_t stream, int sub, bool semi, dim3 grid, const yuv_args &a, uint8_t *dst)
{
    // the profile names say what a dispatch moved: input sample size, subsampling, output sample size
    switch (sub) {
        case CE_YUV_444: launch_layout<BPS, OUT16, CE_YUV_444>(ctx, stream, BPS == 1 ? (OUT16 ? "yuv444_8_deep" : "yuv444_8") : (OUT16 ? "yuv444_16_deep" : "yuv444_16"), semi, grid, a, dst); break;
        case CE_YUV_422: launch_layout<BPS, OUT16, CE_YUV_422>(ctx, stream, BPS == 1 ? (OUT16 ? "yuv422_8_deep" : "yuv422_8") : (OUT16 ? "yuv422_16_deep" : "yuv422_16"), semi, grid, a, dst); break;
        case CE_YUV_420: launch_layout<BPS, OUT16, CE_YUV_420>(ctx, stream, BPS == 1 ? (OUT16 ? "yuv420_8_deep" : "yuv420_8") : (OUT16 ? "yuv420_16_deep" : "yuv420_16"), semi, grid, a, dst); break;
        default: launch_layout<BPS, OUT16, CE_YUV_400>(ctx, stream, BPS == 1 ? (OUT16 ? "yuv400_8_deep" : "yuv400_8") : (OUT16 ? "yuv400_16_deep" : "yuv400_16"), semi, grid, a, dst); break;
    }
}

}  // namespace

int ce_launch_yuv(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, bool out16, uint32_t depth_out)
{
    if (w == 0 || h == 0) return CE_OK;
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    if (blocks > 0x7fffffffu) {
        ctx->err = "Y'CbCr ingest: image too large for one launch";
        return CE_ERR_INVALID_ARG;
    }
    yuv_args a{};
    ce_fill_yuv_args(a, src, w, h, ((int64_t)1 << depth_out) - 1);
    const dim3 grid((uint32_t)blocks);
    const bool semi = src.layout == CE_YUV_SEMIPLANAR;
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    if (src.depth == 8) {
        if (out16) launch_sub<1, true>(ctx, stream, src.subsampling, semi, grid, a, dst);
        else launch_sub<1, false>(ctx, stream, src.subsampling, semi, grid, a, dst);
    } else {
        if (out16) launch_sub<2, true>(ctx, stream, src.subsampling, semi, grid, a, dst);
        else launch_sub<2, false>(ctx, stream, src.subsampling, semi, grid, a, dst);
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
