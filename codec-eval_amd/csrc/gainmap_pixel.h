// One pixel of the gain-map ingest (include/ce_metrics.h: the definition of ce_batch_set_*_gainmap): the base's three gathers
// from its CICP transfer table, the map's four neighbours around the pixel's centre - centres aligned, edges clamped, in
// integers - the bilinear interpolation of the host-built log2-gain table in f64, gm_exp2, one f64 product and difference per
// channel rounded once to f32, then cicp_pixel.h's matrix and clamp.  Unlike cicp_px and hlg_px this pixel needs its
// position, so it has a frame of its own (gainmap_kernel.h).  gm_exp2 is a fixed sequence of IEEE f64 operations like
// hlg_pow, whose second half it shares (hlg_pixel.h: exp_times_pow2); tests/gainmap_restatement.py runs the same sequence in
// numpy.  Host-compilable like the headers it includes, and compiled with -ffp-contract=off, which holds for f64 too.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

#include "cicp_pixel.h"
#include "hlg_pixel.h"

namespace {

struct gainmap_args {
    cicp_args c;         // src, dst, n_pixels, table (the base's transfer table), maxv and m, as the CICP pixel reads them
    const uint8_t *map;  // gw x gh x NCH samples, tightly packed
    const double *ytab;  // NCH tables of 256 log2 gains, W folded in (ce_gainmap_tables)
    uint32_t w, h;       // the base's shape: w * h == c.n_pixels
    uint32_t gw, gh;     // the map's: 1 <= gw <= w, 1 <= gh <= h
    double kb[3];        // base_offset per output channel (a single-channel map: index 0 three times)
    double ka[3];        // alternate_offset, likewise
};

// 2^y for |y| <= 1000: n = rint(y), f = (y - n) ln2 in [-ln2 / 2, ln2 / 2], exp f * 2^n through hlg_pow's second half.  An
// integral y gives f = 0 and exactly that power of two.  Within 1e-15 relative of the real 2^y on [-16, 16].
__device__ __forceinline__ double gm_exp2(double y)
{
    const double n = __builtin_rint(y);
    const double f = (y - n) * 0.6931471805599453;
    return exp_times_pow2(f, n);
}

// one axis of step 2: pixel p of n, map size gn -> the two map indices and the fraction between them
__device__ __forceinline__ void gainmap_axis(uint32_t p, uint32_t n, uint32_t gn, uint32_t &i0, uint32_t &i1, double &f)
{
    const int64_t two_n = 2 * (int64_t)n, hi = ((int64_t)gn - 1) * two_n;
    int64_t c = (2 * (int64_t)p + 1) * (int64_t)gn - (int64_t)n;
    c = c < 0 ? 0 : (c > hi ? hi : c);
    const int64_t i = c / two_n;
    i0 = (uint32_t)i;
    i1 = i0 + 1 < gn ? i0 + 1 : gn - 1;
    f = (double)(c - i * two_n) / (double)two_n;
}

// a + f (b - a): three separately rounded operations
__device__ __forceinline__ double gainmap_lerp(double a, double b, double f)
{
    const double d = b - a;
    const double s = f * d;
    return a + s;
}

// steps 1 - 6 of the definition for the pixel at (x, y) with code values r, g, b
template <int NCH, bool MATRIX>
__device__ __forceinline__ void gainmap_pixel(const gainmap_args &a, uint32_t x, uint32_t y, uint32_t r, uint32_t g, uint32_t b, float (&o)[3])
{
    const uint32_t maxv = a.c.maxv;
    const float t[3] = {a.c.table[r < maxv ? r : maxv], a.c.table[g < maxv ? g : maxv], a.c.table[b < maxv ? b : maxv]};
    uint32_t x0, x1, y0, y1;
    double fx, fy;
    gainmap_axis(x, a.w, a.gw, x0, x1, fx);
    gainmap_axis(y, a.h, a.gh, y0, y1, fy);
    const uint8_t *row0 = a.map + (size_t)y0 * a.gw * NCH, *row1 = a.map + (size_t)y1 * a.gw * NCH;
    double gain[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const double *yt = a.ytab + 256 * c;
        const double top = gainmap_lerp(yt[row0[(size_t)x0 * NCH + c]], yt[row0[(size_t)x1 * NCH + c]], fx);
        const double bottom = gainmap_lerp(yt[row1[(size_t)x0 * NCH + c]], yt[row1[(size_t)x1 * NCH + c]], fx);
        gain[c] = gm_exp2(gainmap_lerp(top, bottom, fy));
    }
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lifted = (double)t[c] + a.kb[c];
        const double scaled = lifted * gain[NCH == 1 ? 0 : c];
        v[c] = (float)(scaled - a.ka[c]);
    }
    cicp_matrix_clamp<MATRIX>(a.c, v[0], v[1], v[2], o);
}

}  // namespace
