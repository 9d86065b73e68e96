// HLG ingest on the device (include/ce_metrics.h: ce_batch_set_*_hlg, ce_hlg_to_linear): a decoder's
// RGB code values in BT.2100 HLG -> display light through the inverse OETF and the OOTF -> linear light with BT.709 / sRGB
// primaries, as packed f32 RGB in a slot of a linear batch.  One launch per image, in cicp.hip's frame: sample -> host-built
// inverse-OETF table (the curve is never evaluated here) -> scene luminance in f64 -> Ys^(gamma - 1) through hlg_pow, a fixed
// sequence of correctly rounded f64 operations (hlg_pixel.h) -> one f32 scale -> optional 3 x 3 primaries matrix -> clamp of a
// linear image, everything compiled with -ffp-contract=off so that tests/hlg_restatement.py reproduces it bit for bit.
//
// 3-8 bytes in and 12 bytes out per pixel, as cicp.hip; on top of its gather and stores a pixel costs about 70 f64
// operations, two of them divisions.  A thread owns four pixels; the table stays in global memory at every depth.  No LDS,
// no scratch.
#include "ce_internal.h"

#include "hlg_kernel.h"

template <int FMT>
static void launch_hlg(ce_ctx *ctx, hipStream_t stream, const char *name, const char *name_m, dim3 grid, const hlg_args &a, bool matrix)
{
    if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_hlg<FMT, true>), grid, dim3(kCicpBlock), 0, a);
    else CE_LAUNCH_ON(ctx, stream, name, (k_hlg<FMT, false>), grid, dim3(kCicpBlock), 0, a);
}

int ce_launch_hlg(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const float *d_table,
                  uint32_t maxv, const float *matrix, const double params[5])
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu || !d_table) {
        ctx->err = "HLG ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    hlg_args a{};
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    ce_fill_cicp_args(a.c, d_dst, d_table, maxv, matrix);
    a.kr = params[0], a.kg = params[1], a.kb = params[2], a.gm1 = params[3], a.a = params[4];
    const dim3 grid((uint32_t)blocks);
    switch (format) {
        case CE_PIXEL_RGB8: launch_hlg<CE_PIXEL_RGB8>(ctx, stream, "hlg_rgb8", "hlg_rgb8_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGBA8: launch_hlg<CE_PIXEL_RGBA8>(ctx, stream, "hlg_rgba8", "hlg_rgba8_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGB16: launch_hlg<CE_PIXEL_RGB16>(ctx, stream, "hlg_rgb16", "hlg_rgb16_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGBA16: launch_hlg<CE_PIXEL_RGBA16>(ctx, stream, "hlg_rgba16", "hlg_rgba16_m", grid, a, matrix != nullptr); break;
        default: ctx->err = "HLG ingest: format must be RGB8, RGBA8, RGB16 or RGBA16"; return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
