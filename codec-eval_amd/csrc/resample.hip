// The resampler behind ce_resample_rgb8 / ce_batch_resample (include/ce_metrics.h): the two passes
// of a separable fixed-point convolution over packed RGB8, a horizontal pass over rows and a vertical pass over the
// image between them.  All arithmetic is integer - 22-bit weights built on the host (ce_tables.cpp), an int32
// accumulator, one arithmetic shift, a clip - so the output is a function of the tables and the input bytes alone.
//
// Both kernels are streams: a block covers kTileBytes consecutive bytes of ONE output row and a thread one dword of
// them, aligned in the destination slab (an image starts at any byte of its slab, a row at any byte of its image), so a
// wave's 64 stores are 256 consecutive bytes.  Only the first and the last dword of a tile can be partial; those are
// stored byte by byte.
//   horizontal  the taps differ from pixel to pixel: the block stages the tables of its <= kTilePixels output pixels in
//               LDS, tap-major ([tap][pixel]: a wave's lanes read consecutive words, the three bytes of a pixel the same
//               one), and falls back to the global table when a tile's taps exceed kLdsInts (scales beyond ~5)
//   vertical    every byte of an output row uses the same taps: they are indexed by the block alone, so the compiler
//               loads them through the scalar cache; a thread reads its four source bytes of a row as one (unaligned) word
// The device code and the geometry of a launch are resample_kernel.h's, which a test also compiles for the host; here are
// the kernels' entry points and the launches.
#include "ce_internal.h"

#include "resample_kernel.h"

namespace {

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_resample_h(pass_geom g, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    extern __shared__ int32_t s_tab[];  // LDS: [2 + ksize][kTilePixels]
    const place p = find_place(g);
    if (LDS) {
        resample_h_stage(p, tab, n_out, ksize, s_tab);
        __syncthreads();
    }
    resample_h_body<LDS>(g, p, tab, n_out, ksize, s_tab);
}

__global__ __launch_bounds__(kThreads) void k_resample_v(pass_geom g, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    resample_v_body(g, tab, n_out, ksize);
}

}  // namespace

int ce_launch_resample(ce_ctx *ctx, hipStream_t stream, const uint8_t *d_src, size_t src_stride, uint8_t *d_dst, size_t dst_stride,
                       uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, const ce_resample_axis *horiz,
                       const ce_resample_axis *vert, uint8_t *mid)
{
    resample_launch r;
    if (!plan_resample(d_src, src_stride, d_dst, dst_stride, w, h, out_w, out_h, n, horiz != nullptr, vert != nullptr,
                       horiz ? horiz->ksize : 0, mid, &r)) {
        ctx->err = "resample: too many tiles for one launch";
        return CE_ERR_INVALID_ARG;
    }
    const auto *htab = static_cast<const int32_t *>(horiz ? horiz->d : nullptr), *vtab = static_cast<const int32_t *>(vert ? vert->d : nullptr);
    if (horiz) {
        if (r.h.lds)
            CE_LAUNCH_ON(ctx, stream, "resample_h", k_resample_h<true>, dim3(r.h.grid), dim3(kThreads), r.h.lds_bytes, r.h.g, htab, out_w,
                         horiz->ksize);
        else
            CE_LAUNCH_ON(ctx, stream, "resample_h_wide", k_resample_h<false>, dim3(r.h.grid), dim3(kThreads), 0, r.h.g, htab, out_w,
                         horiz->ksize);
    }
    if (vert) CE_LAUNCH_ON(ctx, stream, "resample_v", k_resample_v, dim3(r.v.grid), dim3(kThreads), 0, r.v.g, vtab, out_h, vert->ksize);
    return ce_resample_launched(ctx);
}
