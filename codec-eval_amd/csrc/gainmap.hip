// Ingest of gain-map images on the device (include/ce_metrics.h: ce_batch_set_*_gainmap, ce_gainmap_to_linear; DESIGN.md
// section 21): an SDR base image's RGB code values, read by a CICP description as cicp.hip reads them, times the gain that a
// small 8-bit map and a few numbers of metadata describe -> the HDR rendition as packed f32 RGB in a slot of a linear batch.
// One launch per image, one frame (gainmap_kernel.h: k_gainmap) and one pixel (gainmap_pixel.h): sample -> host-built
// transfer table; the map's four neighbours around the pixel's centre -> host-built table of log2 gains (the metadata's
// gamma, range and weight never reach the device) -> bilinear interpolation in f64 -> gm_exp2, a fixed sequence of correctly
// rounded f64 operations -> (t + base_offset) * gain - alternate_offset, rounded once to f32 -> cicp.hip's matrix and clamp.
// Everything is compiled with -ffp-contract=off, so numpy reproduces it bit for bit (tests/gainmap_restatement.py).
//
// A streaming kernel of 3-8 bytes in and 12 bytes out per pixel like the other two, with per map channel about 45 f64
// operations on top - two interpolations' worth of adds and multiplies and the 16-step Horner form - and two f64 divisions
// per pixel for the fractions.  A thread owns four consecutive pixels, with k_tagged's loads and stores.  The map and the
// tables stay in global memory: 2 or 6 KB of tables live in the vector L1, and the map's samples are shared by the pixels
// around them.  No LDS, no scratch.
#include "ce_internal.h"

#include "gainmap_kernel.h"
#include "packed_ladder.h"

int ce_launch_gainmap(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, const uint8_t *d_side, float *d_dst, uint32_t w, uint32_t h,
                      const ce_gainmap_plan &plan)
{
    const size_t n_pixels = (size_t)w * h;
    if (n_pixels == 0) return CE_OK;
    const size_t blocks = std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);
    const bool shape_ok = (plan.channels == 1 || plan.channels == 3) && plan.gw >= 1 && plan.gw <= w && plan.gh >= 1 && plan.gh <= h;
    if (blocks > 0x7fffffffu || !plan.base.d_table || !d_side || !shape_ok) {
        ctx->err = "gain-map ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    gainmap_args a{};
    a.c.src = d_src, a.c.dst = d_dst, a.c.n_pixels = n_pixels, a.c.table = plan.base.d_table, a.c.maxv = plan.base.maxv;
    if (plan.base.has_matrix)
        for (int i = 0; i < 9; i++) a.c.m[i] = plan.base.m[i];
    a.ytab = reinterpret_cast<const double *>(d_side), a.map = d_side + plan.table_bytes();
    a.w = w, a.h = h, a.gw = plan.gw, a.gh = plan.gh;
    for (int c = 0; c < 3; c++) a.kb[c] = plan.base_offset[c], a.ka[c] = plan.alternate_offset[c];
    const dim3 grid((uint32_t)blocks);
    const bool three = plan.channels == 3, matrix = plan.base.has_matrix;
    const char *suffix = three ? (matrix ? "_3_m" : "_3") : (matrix ? "_1_m" : "_1");
    const bool known = packed_ladder(format, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        const packed_profile_name name("gainmap", "", FMT, suffix);
        if (three && matrix) CE_LAUNCH_ON(ctx, stream, name.s, (k_gainmap<FMT, 3, true>), grid, dim3(kCicpBlock), 0, a);
        else if (three) CE_LAUNCH_ON(ctx, stream, name.s, (k_gainmap<FMT, 3, false>), grid, dim3(kCicpBlock), 0, a);
        else if (matrix) CE_LAUNCH_ON(ctx, stream, name.s, (k_gainmap<FMT, 1, true>), grid, dim3(kCicpBlock), 0, a);
        else CE_LAUNCH_ON(ctx, stream, name.s, (k_gainmap<FMT, 1, false>), grid, dim3(kCicpBlock), 0, a);
    });
    if (!known) {
        ctx->err = "gain-map ingest: format must be RGB8, RGBA8, RGB16 or RGBA16";
        return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
