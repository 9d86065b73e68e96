// CICP ingest on the device (include/ce_metrics.h: ce_batch_set_*_cicp, ce_cicp_to_linear): a
// decoder's RGB code values tagged with H.273 colour primaries and transfer characteristics -> linear light with BT.709 /
// sRGB primaries, as packed f32 RGB in a slot of a linear batch.  One launch per image: sample -> host-built transfer table
// (the curve is never evaluated here) -> optional 3 x 3 primaries matrix in separately rounded f32 products and sums
// (-ffp-contract=off, so numpy float32 reproduces it bit for bit) -> NaN / range clamp of a linear image.  The same file
// holds the CE_PIXEL_RGB_F32 upload's clamp pass.
//
// A streaming kernel of 3-8 bytes in and 12 bytes out per pixel.  A thread owns four pixels: aligned dword / 8- / 16-byte
// loads from the staging image and three 16-byte stores where the slot is 16-byte aligned (slot k of the slab starts at
// k * w * h * 12 bytes, so every slot of an image with w * h a multiple of 4 and slot 0 of any image), twelve 4-byte stores
// otherwise - a branch the whole launch takes alike.  The transfer table stays in global memory at every depth: the 1, 4
// and 16 KB tables live in the vector L1 after the first touch, the 256 KB table of depth 16 in L2 (the gather section 11
// measured as small beside the front ends' arithmetic), and one code path serves all four.  No LDS, no scratch.
#include "ce_internal.h"

#include "cicp_kernel.h"

int ce_launch_linear_sanitise(ce_ctx *ctx, hipStream_t stream, const float *d_src, float *d_dst, size_t n_samples)
{
    if (n_samples == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_samples / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu) {
        ctx->err = "linear upload: image too large";
        return CE_ERR_INVALID_ARG;
    }
    CE_LAUNCH_ON(ctx, stream, "ingest_linear_f32", k_linear_sanitise, dim3((uint32_t)blocks), dim3(kCicpBlock), 0, d_src, d_dst, n_samples);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

template <int FMT>
static void launch_cicp(ce_ctx *ctx, hipStream_t stream, const char *name, const char *name_m, dim3 grid, const cicp_args &a, bool matrix)
{
    if (matrix) CE_LAUNCH_ON(ctx, stream, name_m, (k_cicp<FMT, true>), grid, dim3(kCicpBlock), 0, a);
    else CE_LAUNCH_ON(ctx, stream, name, (k_cicp<FMT, false>), grid, dim3(kCicpBlock), 0, a);
}

int ce_launch_cicp(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, float *d_dst, size_t n_pixels, const float *d_table,
                   uint32_t maxv, const float *matrix)
{
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    if (blocks > 0x7fffffffu || !d_table) {
        ctx->err = "CICP ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    cicp_args a{};
    a.src = d_src, a.n_pixels = n_pixels;
    ce_fill_cicp_args(a, d_dst, d_table, maxv, matrix);
    const dim3 grid((uint32_t)blocks);
    switch (format) {
        case CE_PIXEL_RGB8: launch_cicp<CE_PIXEL_RGB8>(ctx, stream, "cicp_rgb8", "cicp_rgb8_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGBA8: launch_cicp<CE_PIXEL_RGBA8>(ctx, stream, "cicp_rgba8", "cicp_rgba8_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGB16: launch_cicp<CE_PIXEL_RGB16>(ctx, stream, "cicp_rgb16", "cicp_rgb16_m", grid, a, matrix != nullptr); break;
        case CE_PIXEL_RGBA16: launch_cicp<CE_PIXEL_RGBA16>(ctx, stream, "cicp_rgba16", "cicp_rgba16_m", grid, a, matrix != nullptr); break;
        default: ctx->err = "CICP ingest: format must be RGB8, RGBA8, RGB16 or RGBA16"; return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
