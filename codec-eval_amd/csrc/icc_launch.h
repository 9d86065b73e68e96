// The launcher of an ICC profile's pixel over packed code values, once for icc.hip (icc_pixel.h's icc_px<MATRIX>, icc_args)
// and icc_lut.hip (icc_lut_pixel.h's icc_lut_px<TETRA>, icc_lut_args).  Two translation units instantiate it, so that a
// parallel build compiles the slow LUT pixel beside the other.
#pragma once

#include "ce_internal.h"

#include "icc_kernel.h"
#include "over_linear_kernel.h"
#include "packed_ladder.h"

// One launch of Px<second> over n_pixels pixels: cicp_kernel.h's k_tagged into a linear slot, icc_kernel.h's k_icc_encode into a
// u8 or u16 slot, over_linear_kernel.h's k_tagged_over with `ov` (whose plan, format and slot kind ce_launch_icc has checked).
// fill(a) puts the profile into the pixel's Args; the profile name is <stem>{_lin|_u8|_u16|_over}_<format><suffix>.
template <template <bool> class Px, class Args, class Fill>
int icc_launch(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, void *d_dst, size_t n_pixels, const ce_icc_pixel &px,
               const ce_over_plan *ov, bool second, const char *stem, const char *suffix, Fill fill)
{
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    const bool integer = px.depth_out != 0;
    if (blocks > 0x7fffffffu || !px.d_tables || !d_src || !d_dst || (integer && !px.d_thr)) {
        ctx->err = "ICC ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    Args a{};
    a.c.src = d_src, a.c.n_pixels = n_pixels;
    a.c.dst = integer ? nullptr : static_cast<float *>(d_dst);
    fill(a);
    const uint32_t top = integer ? 1u << (px.depth_out - 1) : 0u;
    const char *slot = ov ? "_over" : !integer ? "_lin" : px.out16 ? "_u16" : "_u8";
    const dim3 grid((uint32_t)blocks), block(kCicpBlock);
    over_args o{};
    if (ov) ce_fill_over_args(o, *ov);
    auto launch = [&](auto fmt, const auto &pixel) {
        constexpr int FMT = decltype(fmt)::value;
        using P = std::decay_t<decltype(pixel)>;
        const packed_profile_name name(stem, slot, FMT, suffix);
        if (ov) {
            if constexpr (packed_has_alpha(FMT)) CE_LAUNCH_ON(ctx, stream, name.s, (k_tagged_over<FMT, P>), grid, block, 0, pixel, o);
        } else if (!integer) {
            CE_LAUNCH_ON(ctx, stream, name.s, (k_tagged<FMT, P>), grid, block, 0, pixel);
        } else if (px.out16) {
            CE_LAUNCH_ON(ctx, stream, name.s, (k_icc_encode<FMT, true, P>), grid, block, 0, pixel, d_dst, px.d_thr, top);
        } else {
            CE_LAUNCH_ON(ctx, stream, name.s, (k_icc_encode<FMT, false, P>), grid, block, 0, pixel, d_dst, px.d_thr, top);
        }
    };
    const bool known = packed_ladder(format, [&](auto fmt) {
        if (second) launch(fmt, Px<true>{a});
        else launch(fmt, Px<false>{a});
    });
    if (!known) {
        ctx->err = "ICC ingest: format must be RGB8, RGBA8, RGB16 or RGBA16";
        return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
