// Alpha compositing on the device (include/ce_metrics.h: ce_batch_set_*_over, ce_composite_rgba*):
// a decoder's straight-alpha RGBA image, source-over onto K opaque solid colours, into K consecutive slots of a resident
// batch.  One launch per uploaded image: a pixel is read once and its K composites are written from registers.  The
// arithmetic is the header's, on the encoded sample values, in unsigned 32-bit integers with an exact division.
//
// Not part of this: premultiplied alpha, linear-light blending (the convention of libjxl's command-line tools), patterned
// (checkerboard) backgrounds, dssim-core's own alpha handling, CE_PIXEL_RGBA16_10BIT, device-resident sources, ce_ref_*
// handles, ce_eval_batch, ce_eval_batch_lut and ce_batch_resample*.
//
// A streaming kernel of 4 + 3 K (u8) or 8 + 6 K (u16) bytes per pixel, shaped like k_ingest_deep: a thread owns the pixels
// of 48 output bytes (16 of a u8 slot, 8 of a u16 slot), reads them in 16-byte loads (RGBA8: 4 or 2, RGBA16: 4) and stores
// each slot's 48 bytes as three 16-byte words where that slot's address allows.  Slot k of an RGB8 slab starts at
// k * w * h * 3 bytes, so the alignment differs from slot to slot of one launch: each falls back on its own to 8-, 4-, 2-
// or 1-byte stores (a branch that all threads of the launch take alike).  The tail of fewer than 16 / 8 pixels goes sample
// by sample.  No LDS, no scratch.
#include "ce_internal.h"

#include "alpha_kernel.h"

int ce_launch_alpha(ce_ctx *ctx, hipStream_t stream, const void *d_src, bool src16, void *d_dst, bool dst16, uint32_t depth,
                    size_t n_pixels, uint32_t n_bg, const uint16_t *backgrounds)
{
    if (n_pixels == 0) return CE_OK;
    const size_t groups = n_pixels / (dst16 ? 8 : 16), blocks = std::max<size_t>((groups + kAlphaBlock - 1) / kAlphaBlock, 1);
    if (n_bg == 0 || n_bg > CE_MAX_BACKGROUNDS || blocks > 0x7fffffffu || (src16 && !dst16) || (!src16 && depth != 8)) {
        ctx->err = "alpha compositing: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    alpha_args a{};
    a.src = d_src, a.dst = static_cast<uint8_t *>(d_dst);
    a.slot_bytes = n_pixels * 3 * (dst16 ? 2 : 1), a.n_pixels = n_pixels, a.n_bg = n_bg;
    for (uint32_t k = 0; k < n_bg; k++)
        for (int c = 0; c < 3; c++) a.bg[k][c] = backgrounds[3 * k + c];
    const dim3 grid((uint32_t)blocks), block(kAlphaBlock);
    if (!dst16) CE_LAUNCH_ON(ctx, stream, "alpha_rgba8", (k_alpha<false, false, 8>), grid, block, 0, a);
    else if (!src16) CE_LAUNCH_ON(ctx, stream, "alpha_rgba8_deep", (k_alpha<false, true, 8>), grid, block, 0, a);
    else if (depth == 8) CE_LAUNCH_ON(ctx, stream, "alpha_rgba16_deep", (k_alpha<true, true, 8>), grid, block, 0, a);
    else if (depth == 10) CE_LAUNCH_ON(ctx, stream, "alpha_rgba16_deep", (k_alpha<true, true, 10>), grid, block, 0, a);
    else if (depth == 12) CE_LAUNCH_ON(ctx, stream, "alpha_rgba16_deep", (k_alpha<true, true, 12>), grid, block, 0, a);
    else if (depth == 16) CE_LAUNCH_ON(ctx, stream, "alpha_rgba16_deep", (k_alpha<true, true, 16>), grid, block, 0, a);
    else {
        ctx->err = "alpha compositing: depth must be 8, 10, 12 or 16";
        return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
