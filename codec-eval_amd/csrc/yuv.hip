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
#include "yuv_ladder.h"

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
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    // the profile names say what a dispatch moved: subsampling, input sample size, _deep for u16 output
    yuv_ladder(src.depth == 8, src.subsampling, src.layout == CE_YUV_SEMIPLANAR, [&](auto bps, auto sub, auto semi) {
        constexpr int BPS = decltype(bps)::value, SUB = decltype(sub)::value;
        constexpr bool SEMI = decltype(semi)::value;
        if (out16) CE_LAUNCH_ON(ctx, stream, yuv_profile_name(SUB, BPS, "_deep").s, (k_yuv<BPS, true, SUB, SEMI>), grid, dim3(64), 0, a, dst);
        else CE_LAUNCH_ON(ctx, stream, yuv_profile_name(SUB, BPS, "").s, (k_yuv<BPS, false, SUB, SEMI>), grid, dim3(64), 0, a, dst);
    });
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
