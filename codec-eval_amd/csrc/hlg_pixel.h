// One pixel of the HLG ingest (include/ce_metrics.h: the definition of ce_batch_set_*_hlg), and hlg_px, the pixel as the type
// that cicp_kernel.h's k_tagged and yuv_cicp_kernel.h's k_yuv_tagged take in cicp_px's place: three gathers from the host-built inverse-OETF table, the scene luminance in f64, the OOTF's
// Ys^(gamma - 1) through hlg_pow, one f32 scale per channel, then cicp_pixel.h's matrix and clamp.  hlg_pow is a fixed
// sequence of IEEE f64 additions, multiplications, divisions, integer work on the exponent bits and one round-to-nearest,
// each correctly rounded on the device and on the host alike; tests/hlg_restatement.py runs the same sequence in numpy.
// Host-compilable like the headers that include it, and compiled with -ffp-contract=off, which holds for f64 too.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

#include "cicp_pixel.h"

namespace {

struct hlg_args {
    cicp_args c;        // src, dst, n_pixels, table (the inverse OETF, maxv + 1 entries), maxv and m, as the CICP pixel reads them
    double kr, kg, kb;  // the Y row of the f64 XYZ <- src matrix of the tagged primaries
    double gm1;         // system gamma - 1
    double a;           // peak_nits / white_nits
};

// exp(f) * 2^n for |f| <= ln2 / 2 and an integral n with 2^n normal: exp f as the degree-14 Taylor series in Horner form from
// 1 / 14! down, times 2^n built from bits.  The second half of hlg_pow, and of gainmap_pixel.h's gm_exp2.
__device__ __forceinline__ double exp_times_pow2(double f, double n)
{
    double q = 1.0 / 87178291200.0;  // 1 / 14!
    q = q * f + 1.0 / 6227020800.0;
    q = q * f + 1.0 / 479001600.0;
    q = q * f + 1.0 / 39916800.0;
    q = q * f + 1.0 / 3628800.0;
    q = q * f + 1.0 / 362880.0;
    q = q * f + 1.0 / 40320.0;
    q = q * f + 1.0 / 5040.0;
    q = q * f + 1.0 / 720.0;
    q = q * f + 1.0 / 120.0;
    q = q * f + 1.0 / 24.0;
    q = q * f + 1.0 / 6.0;
    q = q * f + 1.0 / 2.0;
    q = q * f + 1.0;
    q = q * f + 1.0;
    const uint64_t sbits = (uint64_t)((int64_t)n + 1023) << 52;
    double scale;
    __builtin_memcpy(&scale, &sbits, 8);
    return q * scale;
}

// x^g for a normal x > 0.  x = m 2^e with m in [sqrt(1/2), sqrt(2)); ln m = 2 t P(t^2) with t = (m - 1) / (m + 1) and P the
// odd-reciprocal series to 1/21 in Horner form; y = g (ln m + e ln2); n = rint(y / ln2), f = y - n ln2 in [-ln2 / 2, ln2 / 2];
// exp f as the degree-14 Taylor series in Horner form; times 2^n built from bits.  Within 5e-15 relative of the real power
// for x in [2^-60, 4] and g in [-0.4, 0.6]; g = 0 gives exactly 1.  The quotients of literals are folded by the compiler,
// correctly rounded.
__device__ __forceinline__ double hlg_pow(double x, double g)
{
    constexpr double kLn2 = 0.6931471805599453, kSqrt2 = 1.4142135623730951;
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    int64_t e = (int64_t)((bits >> 52) & 0x7ffu) - 1023;
    const uint64_t mbits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &mbits, 8);
    if (m >= kSqrt2) {
        m = m * 0.5;
        e = e + 1;
    }
    const double t = (m - 1.0) / (m + 1.0);
    const double t2 = t * t;
    double p = 1.0 / 21.0;
    p = p * t2 + 1.0 / 19.0;
    p = p * t2 + 1.0 / 17.0;
    p = p * t2 + 1.0 / 15.0;
    p = p * t2 + 1.0 / 13.0;
    p = p * t2 + 1.0 / 11.0;
    p = p * t2 + 1.0 / 9.0;
    p = p * t2 + 1.0 / 7.0;
    p = p * t2 + 1.0 / 5.0;
    p = p * t2 + 1.0 / 3.0;
    p = p * t2 + 1.0;
    const double ln_m = (2.0 * t) * p;
    const double y = g * (ln_m + (double)e * kLn2);
    const double n = __builtin_rint(y / kLn2);
    const double f = y - n * kLn2;
    return exp_times_pow2(f, n);
}

// steps 1 - 5 of the definition: e = table[min(v, maxv)]; ys = (kR e_r + kG e_g) + kB e_b in f64; k = (float)(A ys^(gamma-1)),
// 0 where ys is 0; d = k e in f32; the primaries matrix and the clamp of a linear image
template <bool MATRIX>
__device__ __forceinline__ void hlg_pixel(const hlg_args &a, uint32_t r, uint32_t g, uint32_t b, float (&o)[3])
{
    const uint32_t maxv = a.c.maxv;
    const float er = a.c.table[r < maxv ? r : maxv], eg = a.c.table[g < maxv ? g : maxv], eb = a.c.table[b < maxv ? b : maxv];
    const double pr = a.kr * (double)er, pg = a.kg * (double)eg, pb = a.kb * (double)eb;
    const double srg = pr + pg;
    const double ys = srg + pb;
    const double s = ys > 0.0 ? hlg_pow(ys, a.gm1) : 0.0;
    const float k = (float)(a.a * s);
    const float dr = k * er, dg = k * eg, db = k * eb;
    cicp_matrix_clamp<MATRIX>(a.c, dr, dg, db, o);
}

// cicp_px's counterpart: on top of its gather, matrix and clamp a pixel costs about 70 f64 operations, two of them divisions
template <bool MATRIX>
struct hlg_px {
    hlg_args a;
    __device__ __forceinline__ const cicp_args &frame() const { return a.c; }
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t g, uint32_t b, float (&o)[3]) const { hlg_pixel<MATRIX>(a, r, g, b, o); }
};

}  // namespace
