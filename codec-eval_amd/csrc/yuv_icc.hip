// Y'CbCr planes with an ICC profile straight into a slot of any batch (include/ce_metrics.h: ce_batch_set_*_yuv_icc,
// ce_yuv_icc_to_*): what yuv.hip and icc.hip / icc_lut.hip do behind each other, in one launch per image
// and without the integer RGB image between them.  The definition is the composition of theirs and adds no arithmetic: a
// thread runs yuv_kernel.h's block (8 x 2 pixels: clamped loads, integer upsampling, int64 matrix, clamp to 2^rgb_depth - 1)
// and hands each pixel to the one icc.hip or icc_lut.hip would run - icc_pixel.h's icc_px or icc_lut_pixel.h's icc_lut_px.  A
// linear slot takes yuv_cicp_kernel.h's k_yuv_tagged around that pixel; an RGB8 slot or a deep side takes
// yuv_icc_kernel.h's k_yuv_icc_encode, which searches the sRGB code thresholds for twelve values side by side and stores
// with k_yuv's choice of widths.  Compiled with -ffp-contract=off.
//
// 7 layouts x 2 sample sizes x 4 pixels x 3 slot kinds = 168 kernels, which is why this is a file of its own - and, since the
// LUT pixel makes each of them slow to compile, why the Makefile compiles it three times, once per slot kind
// (-DCE_YUV_ICC_KIND=0, 1, 2: f32, u8, u16), so that a parallel build spreads them.  Each object holds the 56 kernels of its
// kind and ce_launch_yuv_icc_<kind>; object 0 also holds ce_launch_yuv_icc, which picks among them.  1.5 - 6 bytes in and
// 3 - 12 bytes out per pixel; tables, CLUT and thresholds are gathered from global memory as in icc.hip.  No LDS, no scratch.
#include "ce_internal.h"

#include "yuv_icc_kernel.h"
#include "yuv_ladder.h"

namespace {

// the profile names follow yuv.hip's: subsampling, input sample size, then the slot kind and the pixel -
// yuv420_8_icc_lin_m, yuv444_16_icc_u8, yuv422_16_icc_u16_tet
struct icc_suffix {
    char s[16];
    icc_suffix(int kind, const char *pixel) { std::snprintf(s, sizeof s, "_icc_%s%s", kind == 0 ? "lin" : kind == 1 ? "u8" : "u16", pixel); }
};

#ifndef CE_YUV_ICC_KIND
#error "yuv_icc.hip is compiled once per slot kind: -DCE_YUV_ICC_KIND=0 (f32), 1 (u8) or 2 (u16)"
#endif
constexpr int KIND = CE_YUV_ICC_KIND;  // this object's slot kind: 0 a linear slot, 1 a u8 slot, 2 a u16 slot

template <class Pixel>
void launch_pixel(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, const char *pixel, dim3 grid, const yuv_args &y, const Pixel &px, void *d_dst,
                  const float *d_thr, uint32_t top)
{
    const icc_suffix suffix(KIND, pixel);
    yuv_ladder(src.depth == 8, src.subsampling, src.layout == CE_YUV_SEMIPLANAR, [&](auto bps, auto sub, auto semi) {
        constexpr int BPS = decltype(bps)::value, SUB = decltype(sub)::value;
        constexpr bool SEMI = decltype(semi)::value;
        const yuv_profile_name name(SUB, BPS, suffix.s);
        if constexpr (KIND == 0) {
            CE_LAUNCH_ON(ctx, stream, name.s, (k_yuv_tagged<BPS, SUB, SEMI, Pixel>), grid, dim3(64), 0, yuv_px_args<Pixel>{y, px});
        } else {
            const yuv_icc_args<Pixel> k{y, px, static_cast<uint8_t *>(d_dst), d_thr, top};
            CE_LAUNCH_ON(ctx, stream, name.s, (k_yuv_icc_encode<BPS, KIND == 2, SUB, SEMI, Pixel>), grid, dim3(64), 0, k);
        }
    });
}

}  // namespace

#define CE_YUV_ICC_CAT_(a, b) a##b
#define CE_YUV_ICC_CAT(a, b) CE_YUV_ICC_CAT_(a, b)
int CE_YUV_ICC_CAT(ce_launch_yuv_icc_, CE_YUV_ICC_KIND)(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px)
{
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    yuv_args y{};
    ce_fill_yuv_args(y, src, w, h, (int64_t)px.maxv);  // src.k was built for this output depth (yuv_check with depth_out = rgb_depth)
    const uint32_t top = KIND != 0 ? 1u << (px.depth_out - 1) : 0u;
    float *lin = KIND != 0 ? nullptr : static_cast<float *>(d_dst);
    const dim3 grid((uint32_t)blocks);
    // the one place that knows which pixel a plan means
    if (px.lut) {
        icc_lut_args a{};
        a.c.dst = lin;
        ce_fill_icc_lut_args(a, px);
        if (px.lut->tetra) launch_pixel(ctx, stream, src, "_tet", grid, y, icc_lut_px<true>{a}, d_dst, px.d_thr, top);
        else launch_pixel(ctx, stream, src, "_tri", grid, y, icc_lut_px<false>{a}, d_dst, px.d_thr, top);
    } else {
        icc_args a{};
        a.c.dst = lin;
        ce_fill_icc_args(a, px);
        if (px.has_matrix) launch_pixel(ctx, stream, src, "_m", grid, y, icc_px<true>{a}, d_dst, px.d_thr, top);
        else launch_pixel(ctx, stream, src, "", grid, y, icc_px<false>{a}, d_dst, px.d_thr, top);
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

#if CE_YUV_ICC_KIND == 0
int ce_launch_yuv_icc(ce_ctx *ctx, hipStream_t stream, const ce_yuv_dev &src, uint32_t w, uint32_t h, void *d_dst, const ce_icc_pixel &px)
{
    if (w == 0 || h == 0) return CE_OK;
    const size_t groups = (size_t)((w + 7) / 8) * ((h + 1) / 2), blocks = (groups + 63) / 64;
    const bool integer = px.depth_out != 0;
    if (blocks > 0x7fffffffu || !px.d_tables || !d_dst || (integer && !px.d_thr)) {
        ctx->err = "Y'CbCr ICC ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    if (!integer) return ce_launch_yuv_icc_0(ctx, stream, src, w, h, d_dst, px);
    return px.out16 ? ce_launch_yuv_icc_2(ctx, stream, src, w, h, d_dst, px) : ce_launch_yuv_icc_1(ctx, stream, src, w, h, d_dst, px);
}
#endif
