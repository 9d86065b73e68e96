// The device code of the float resampler (resample_f32.hip) and the geometry of its launches, kept free of anything but
// the HIP keywords, min / max and blockIdx / threadIdx as resample_kernel.h is, so that tests/cpp/resample_f32_kernel_host.cpp
// can compile the same text for the host and run it under the host sanitizers.  k_resample_f32_h is split at its barrier
// for that: resample_f32_h_stage fills the LDS, resample_f32_h_body reads it.
//
// The arithmetic (include/ce_metrics.h: ce_resample_linear): acc = 0.0; acc = acc + (double)sample * w_t for the taps in
// ascending order, the product and the sum each rounded to f64 - this text is compiled with -ffp-contract=off on the device
// and on the host - then one rounding to f32.  The last pass of a resample clamps what it stores to +-kLinearMax.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileFloats = kThreads;                // consecutive floats of one output row a block covers, one a lane
constexpr uint32_t kTilePixels = kTileFloats / 3 + 2;     // output pixels those floats can touch
constexpr size_t kLdsBytes = 48 * 1024;                   // taps staged per block at most
constexpr float kLinearMax = 1024.0f;                     // CE_LINEAR_MAX

// geometry of one pass: rows_per_img output rows of out_row_floats per image; strides in floats
struct pass_geom {
    const float *src;
    float *dst;
    size_t src_stride, dst_stride;  // floats between images
    uint32_t src_row_floats, out_row_floats;
    uint32_t rows_per_img;  // output rows of an image
    uint32_t tiles;         // tiles per output row
    bool clamp;             // the last pass of its resample
};

// one pass as it is launched: `grid` blocks of kThreads; the horizontal pass stages its taps in lds_bytes of dynamic LDS
// (`lds`) or, when they do not fit, asks for none and reads the global table
struct pass_launch {
    pass_geom g;
    uint32_t grid;
    size_t lds_bytes;
    bool lds;
};

struct resample_launch {
    bool horiz, vert;
    pass_launch h, v;
};

// the LDS a horizontal tile's taps take - [ksize][kTilePixels] doubles, then first tap and tap count [2][kTilePixels] ints -
// and whether the block stages them there
inline size_t taps_lds_bytes(uint32_t ksize) { return (size_t)kTilePixels * ((size_t)ksize * sizeof(double) + 2 * sizeof(int32_t)); }
inline bool taps_fit_lds(uint32_t ksize) { return ksize != 0 && taps_lds_bytes(ksize) <= kLdsBytes; }

// n images of `rows` output rows: src_w -> dst_w pixels a row (horizontal, ksize taps a pixel) or rows of dst_w = src_w
// pixels (vertical, ksize 0); false when the launch would not fit its 32-bit indices
inline bool plan_pass(const float *src, size_t sstride, uint32_t src_w, float *dst, size_t dstride, uint32_t dst_w, uint32_t rows, uint32_t n,
                      uint32_t ksize, bool clamp, pass_launch *p)
{
    pass_geom *g = &p->g;
    g->src = src, g->dst = dst, g->src_stride = sstride, g->dst_stride = dstride, g->clamp = clamp;
    if ((uint64_t)src_w * 3 > 0x7fffffffull || (uint64_t)dst_w * 3 > 0x7fffffffull - 2 * kTileFloats) return false;
    g->src_row_floats = src_w * 3, g->out_row_floats = dst_w * 3;
    g->rows_per_img = rows;
    g->tiles = (g->out_row_floats + kTileFloats - 1) / kTileFloats;
    if ((uint64_t)g->tiles * rows * n > 0x7fffffffull) return false;
    p->grid = g->tiles * rows * n;
    p->lds = taps_fit_lds(ksize);
    p->lds_bytes = p->lds ? taps_lds_bytes(ksize) : 0;
    return true;
}

// n images of w x h, src_stride floats apart, to out_w x out_h, dst_stride apart.  horizontal: w -> out_w over the h source
// rows, into `mid` (n x h x out_w x 3 floats) when a vertical pass follows; vertical: h -> out_h over rows of out_w pixels
inline bool plan_resample(const float *src, size_t src_stride, float *dst, size_t dst_stride, uint32_t w, uint32_t h, uint32_t out_w,
                          uint32_t out_h, uint32_t n, bool horiz, bool vert, uint32_t ksize_h, float *mid, resample_launch *r)
{
    const bool two = horiz && vert;
    const size_t mid_stride = (size_t)h * out_w * 3;
    r->horiz = horiz, r->vert = vert;
    if (horiz && !plan_pass(src, src_stride, w, two ? mid : dst, two ? mid_stride : dst_stride, out_w, h, n, ksize_h, !vert, &r->h)) return false;
    if (vert && !plan_pass(two ? mid : src, two ? mid_stride : src_stride, out_w, dst, dst_stride, out_w, out_h, n, 0, true, &r->v)) return false;
    return true;
}

// A block's place: its image and output row, the first float `f0` of its tile in that row, and for this thread the float `f`
// of the row it stores (beyond the row in the last tile's tail).
struct place {
    uint32_t img, y, f0, f;
};

__device__ __forceinline__ place find_place(const pass_geom &g)
{
    place p;
    const uint32_t row = blockIdx.x / g.tiles, tile = blockIdx.x - row * g.tiles;
    p.img = row / g.rows_per_img;
    p.y = row - p.img * g.rows_per_img;
    p.f0 = tile * kTileFloats;
    p.f = p.f0 + threadIdx.x;
    return p;
}

__device__ __forceinline__ void store(const pass_geom &g, const place &p, double acc)
{
    float v = (float)acc;
    if (g.clamp) v = v < -kLinearMax ? -kLinearMax : (v > kLinearMax ? kLinearMax : v);
    g.dst[(size_t)p.img * g.dst_stride + (size_t)p.y * g.out_row_floats + p.f] = v;
}

// tab: ce_resample_axis's layout for this resampler.  The int32 head and the weights behind it:
__device__ __forceinline__ const int32_t *tab_head(const double *tab) { return reinterpret_cast<const int32_t *>(tab); }

// Before the barrier: the taps of the block's <= kTilePixels output pixels into s_tab, LDS of taps_lds_bytes(ksize): the
// weights tap-major, [ksize][kTilePixels] (a wave's lanes read consecutive doubles, the three floats of a pixel the same
// one), then [kTilePixels] first taps and [kTilePixels] tap counts.
__device__ __forceinline__ void resample_f32_h_stage(const place &p, const double *__restrict__ tab, uint32_t n_out, uint32_t ksize,
                                                     double *s_tab)
{
    const int32_t *__restrict__ head = tab_head(tab);
    int32_t *s_head = reinterpret_cast<int32_t *>(s_tab + (size_t)ksize * kTilePixels);
    const uint32_t x0 = p.f0 / 3u;
    const uint32_t px = min(kTilePixels, n_out - x0);
    for (uint32_t i = threadIdx.x; i < px; i += kThreads) {
        s_head[i] = head[x0 + i];
        s_head[kTilePixels + i] = head[n_out + x0 + i];
    }
    for (uint32_t i = threadIdx.x; i < px * ksize; i += kThreads) {  // consecutive global doubles -> [tap][pixel]
        const uint32_t xl = i / ksize, t = i - xl * ksize;
        s_tab[t * kTilePixels + xl] = tab[(size_t)n_out + (size_t)x0 * ksize + i];
    }
}

// After it: the thread's float of the output row.  LDS: taps from s_tab as resample_f32_h_stage left them, else from `tab`
// (s_tab is not read).
template <bool LDS>
__device__ __forceinline__ void resample_f32_h_body(const pass_geom &g, const place &p, const double *__restrict__ tab, uint32_t n_out,
                                                    uint32_t ksize, const double *s_tab)
{
    if (p.f >= g.out_row_floats) return;
    const int32_t *__restrict__ head = tab_head(tab);
    const int32_t *s_head = LDS ? reinterpret_cast<const int32_t *>(s_tab + (size_t)ksize * kTilePixels) : nullptr;
    const uint32_t x = p.f / 3u, c = p.f - x * 3u, xl = x - p.f0 / 3u;
    const int32_t xmin = LDS ? s_head[xl] : head[x];
    const int32_t n = LDS ? s_head[kTilePixels + xl] : head[n_out + x];
    const float *s = g.src + (size_t)p.img * g.src_stride + (size_t)p.y * g.src_row_floats + (size_t)xmin * 3u + c;
    const double *k = LDS ? s_tab + xl : tab + (size_t)n_out + (size_t)x * ksize;
    double acc = 0.0;
#pragma unroll 4
    for (int32_t t = 0; t < n; t++) {
        const double wt = LDS ? k[(size_t)t * kTilePixels] : k[t];
        const double prod = (double)s[(size_t)t * 3u] * wt;
        acc = acc + prod;
    }
    store(g, p, acc);
}

// One lane per output float; the row's taps are the same for every thread of the block (the compiler loads them through
// the scalar cache), the source rows are read as the consecutive floats the lanes store.
__device__ __forceinline__ void resample_f32_v_body(const pass_geom &g, const double *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    const place p = find_place(g);
    if (p.f >= g.out_row_floats) return;
    const int32_t *__restrict__ head = tab_head(tab);
    const int32_t ymin = head[p.y], n = head[n_out + p.y];
    const double *__restrict__ k = tab + (size_t)n_out + (size_t)p.y * ksize;
    const float *s = g.src + (size_t)p.img * g.src_stride + (size_t)ymin * g.src_row_floats + p.f;
    double acc = 0.0;
#pragma unroll 4
    for (int32_t t = 0; t < n; t++, s += g.src_row_floats) {
        const double prod = (double)*s * k[t];
        acc = acc + prod;
    }
    store(g, p, acc);
}

}  // namespace
