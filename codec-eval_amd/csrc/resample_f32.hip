// The float resampler behind ce_resample_linear / ce_batch_resample on linear batches (include/ce_metrics.h; DESIGN.md
// section 17): the two passes of the separable convolution of resample.hip over packed f32 RGB in linear light, with the
// normalised f64 weights themselves (ce_tables.cpp: ce_build_resample_table_f64), an f64 accumulator whose products and sums
// are each rounded (-ffp-contract=off, as the whole library is built), and one rounding to f32 per pass - Pillow's
// Image.resize on mode "F", bit for bit.  The last pass clamps its store to +-CE_LINEAR_MAX, the invariant of a linear slab.
//
// Both kernels are streams of 12 bytes a pixel in and out: a block covers kTileFloats consecutive floats of ONE output row
// and a lane one of them (a slab is dword aligned at every image and row, so there is no partial store), a wave's 64 stores
// are 256 consecutive bytes.
//   horizontal  the taps differ from pixel to pixel: the block stages the tables of its <= kTilePixels output pixels in
//               LDS, tap-major, and reads the global table when they exceed kLdsBytes (ksize beyond 69: scales beyond ~11
//               with Lanczos)
//   vertical    every float of an output row uses the same taps, indexed by the block alone; a lane reads its column of
//               the source rows, consecutive lanes consecutive floats
// The device code and the geometry of a launch are resample_f32_kernel.h's, which a test also compiles for the host; here
// are the kernels' entry points and the launches.
#include "ce_internal.h"

#include "resample_f32_kernel.h"

namespace {

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_resample_f32_h(pass_geom g, const double *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    extern __shared__ double s_tab_f64[];  // LDS: taps_lds_bytes(ksize)
    const place p = find_place(g);
    if (LDS) {
        resample_f32_h_stage(p, tab, n_out, ksize, s_tab_f64);
        __syncthreads();
    }
    resample_f32_h_body<LDS>(g, p, tab, n_out, ksize, s_tab_f64);
}

__global__ __launch_bounds__(kThreads) void k_resample_f32_v(pass_geom g, const double *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    resample_f32_v_body(g, tab, n_out, ksize);
}

}  // namespace

static_assert(kLinearMax == CE_LINEAR_MAX, "the kernel header restates CE_LINEAR_MAX");

int ce_launch_resample_f32(ce_ctx *ctx, hipStream_t stream, const float *d_src, size_t src_stride, float *d_dst, size_t dst_stride,
                           uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, const ce_resample_axis *horiz,
                           const ce_resample_axis *vert, float *mid)
{
    resample_launch r;
    if (!plan_resample(d_src, src_stride, d_dst, dst_stride, w, h, out_w, out_h, n, horiz != nullptr, vert != nullptr,
                       horiz ? horiz->ksize : 0, mid, &r)) {
        ctx->err = "resample: too many tiles for one launch";
        return CE_ERR_INVALID_ARG;
    }
    const auto *htab = static_cast<const double *>(horiz ? horiz->d : nullptr), *vtab = static_cast<const double *>(vert ? vert->d : nullptr);
    if (horiz) {
        if (r.h.lds)
            CE_LAUNCH_ON(ctx, stream, "resample_f32_h", k_resample_f32_h<true>, dim3(r.h.grid), dim3(kThreads), r.h.lds_bytes, r.h.g, htab,
                         out_w, horiz->ksize);
        else
            CE_LAUNCH_ON(ctx, stream, "resample_f32_h_wide", k_resample_f32_h<false>, dim3(r.h.grid), dim3(kThreads), 0, r.h.g, htab, out_w,
                         horiz->ksize);
    }
    if (vert)
        CE_LAUNCH_ON(ctx, stream, "resample_f32_v", k_resample_f32_v, dim3(r.v.grid), dim3(kThreads), 0, r.v.g, vtab, out_h, vert->ksize);
    return ce_resample_launched(ctx);
}
