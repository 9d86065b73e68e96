// One pixel of CIEDE2000 (include/ce_metrics.h: the definition of ce_batch_ciede2000): two table values
// per channel widened to f64, OpenCV's XYZ matrix, CIE Lab, and the colour difference of Sharma, Wu and Dalal (2005) with
// kL = kC = kH = 1, quantised to units of 2^-20.  The cube root, the hue angle, the sines and cosines of degrees and the
// exponential are fixed sequences of IEEE f64 additions, subtractions, multiplications, divisions, square roots, one
// round-to-nearest and integer work on the exponent bits, each correctly rounded on the device and on the host alike - no
// libm, no device math library - and tests/ciede2000_restatement.py runs the same sequences in numpy.  Host-compilable like
// hlg_pixel.h, whose exp_times_pow2 is the second half of the exponential here, and compiled with -ffp-contract=off, which
// holds for f64 too: the device (ciede2000.hip) and ce_ciede2000_pixels (ce_ciede2000_host.cpp) compile this one text.
#pragma once

#include <cstddef>
#include <cstdint>

#include "hlg_pixel.h"

namespace {

// cbrt t for a normal t > 0.  t = m 2^e with m in [1, 2) and e = 3 k + r, r in {0, 1, 2}; y0 = 0.7401 + 0.2599 m, within
// 1.2 % of cbrt m; three Halley steps y <- y (y^3 + 2 m) / (2 y^3 + m), each cubing the relative error; times cbrt(2)^r;
// times 2^k built from bits.  Within 6e-16 relative of the real cube root.
__device__ __forceinline__ double cie_cbrt(double t)
{
    uint64_t bits;
    __builtin_memcpy(&bits, &t, 8);
    const int64_t e3 = (int64_t)((bits >> 52) & 0x7ffu) - 1023 + 3072;
    const uint64_t mbits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &mbits, 8);
    const int64_t k3 = e3 / 3, r = e3 - 3 * k3, k = k3 - 1024;
    double y = 0.7401 + (0.2599 * m);
    const double m2 = m + m;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double y3 = (y * y) * y;
        y = (y * (y3 + m2)) / ((y3 + y3) + m);
    }
    const double c = r == 0 ? 1.0 : r == 1 ? 1.2599210498948732 : 1.5874010519681994;  // cbrt 2, cbrt 4
    const uint64_t sbits = (uint64_t)(k + 1023) << 52;
    double scale;
    __builtin_memcpy(&scale, &sbits, 8);
    return (y * c) * scale;
}

// atan2(b, a) in degrees in [0, 360), 0 at a = b = 0.  t = min(|a|, |b|) / max(|a|, |b|); above tan(pi / 8) the argument is
// (t - 1) / (t + 1) and 45 is added; the odd Taylor series of the arctangent to u^49 in Horner form, times 180 / pi; then the
// octant (90 - d where |b| > |a|), the half plane (180 - d where a < 0) and the sign of b (360 - d where b < 0, and 360 -> 0).
__device__ __forceinline__ double cie_hue_deg(double b, double a)
{
    const double ax = a < 0.0 ? -a : a, ay = b < 0.0 ? -b : b;
    const double mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    if (mx == 0.0) return 0.0;
    const double t = mn / mx;
    const bool big = t > 0.41421356237309503;
    const double u = big ? (t - 1.0) / (t + 1.0) : t;
    const double u2 = u * u;
    double p = 1.0 / 49.0;
    p = (p * u2) + (-1.0 / 47.0);
    p = (p * u2) + (1.0 / 45.0);
    p = (p * u2) + (-1.0 / 43.0);
    p = (p * u2) + (1.0 / 41.0);
    p = (p * u2) + (-1.0 / 39.0);
    p = (p * u2) + (1.0 / 37.0);
    p = (p * u2) + (-1.0 / 35.0);
    p = (p * u2) + (1.0 / 33.0);
    p = (p * u2) + (-1.0 / 31.0);
    p = (p * u2) + (1.0 / 29.0);
    p = (p * u2) + (-1.0 / 27.0);
    p = (p * u2) + (1.0 / 25.0);
    p = (p * u2) + (-1.0 / 23.0);
    p = (p * u2) + (1.0 / 21.0);
    p = (p * u2) + (-1.0 / 19.0);
    p = (p * u2) + (1.0 / 17.0);
    p = (p * u2) + (-1.0 / 15.0);
    p = (p * u2) + (1.0 / 13.0);
    p = (p * u2) + (-1.0 / 11.0);
    p = (p * u2) + (1.0 / 9.0);
    p = (p * u2) + (-1.0 / 7.0);
    p = (p * u2) + (1.0 / 5.0);
    p = (p * u2) + (-1.0 / 3.0);
    p = (p * u2) + 1.0;
    double d = (u * p) * 57.29577951308232;  // 180 / pi
    d = big ? d + 45.0 : d;
    d = ay > ax ? 90.0 - d : d;
    d = a < 0.0 ? 180.0 - d : d;
    d = b < 0.0 ? 360.0 - d : d;
    return d >= 360.0 ? d - 360.0 : d;
}

// sin and cos of x degrees, |x| < 2^31.  n = rint(x / 90); r = x - 90 n, exact, in [-45, 45]; rr = r (pi / 180); the Taylor
// series of the sine to rr^17 and of the cosine to rr^18 in Horner form; the quadrant n mod 4 picks and signs them.
__device__ __forceinline__ void cie_sincos_deg(double x, double &sn, double &cs)
{
    const double n = __builtin_rint(x / 90.0);
    const double r = x - (90.0 * n);
    const double rr = r * 0.017453292519943295;  // pi / 180
    const double r2 = rr * rr;
    double s = 1.0 / 355687428096000.0;  // 1 / 17!
    s = (s * r2) + (-1.0 / 1307674368000.0);
    s = (s * r2) + (1.0 / 6227020800.0);
    s = (s * r2) + (-1.0 / 39916800.0);
    s = (s * r2) + (1.0 / 362880.0);
    s = (s * r2) + (-1.0 / 5040.0);
    s = (s * r2) + (1.0 / 120.0);
    s = (s * r2) + (-1.0 / 6.0);
    s = (s * r2) + 1.0;
    s = rr * s;
    double c = -1.0 / 6402373705728000.0;  // -1 / 18!
    c = (c * r2) + (1.0 / 20922789888000.0);
    c = (c * r2) + (-1.0 / 87178291200.0);
    c = (c * r2) + (1.0 / 479001600.0);
    c = (c * r2) + (-1.0 / 3628800.0);
    c = (c * r2) + (1.0 / 40320.0);
    c = (c * r2) + (-1.0 / 720.0);
    c = (c * r2) + (1.0 / 24.0);
    c = (c * r2) + (-1.0 / 2.0);
    c = (c * r2) + 1.0;
    const int64_t q = (int64_t)n & 3;
    sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
__device__ __forceinline__ double cie_sin_deg(double x)
{
    double s, c;
    cie_sincos_deg(x, s, c);
    return s;
}
__device__ __forceinline__ double cie_cos_deg(double x)
{
    double s, c;
    cie_sincos_deg(x, s, c);
    return c;
}

// exp y for y in [-700, 0]: n = rint(y / ln2), f = y - n ln2, hlg_pixel.h's degree-14 series times 2^n
__device__ __forceinline__ double cie_exp(double y)
{
    constexpr double kLn2 = 0.6931471805599453;
    const double n = __builtin_rint(y / kLn2);
    const double f = y - (n * kLn2);
    return exp_times_pow2(f, n);
}

__device__ __forceinline__ double cie_pow7(double c)
{
    const double c3 = (c * c) * c;
    return (c3 * c3) * c;
}

struct cie_lab {
    double l, a, b;
};

// steps 2 and 3 of the definition: three table values (f32, widened exactly) -> XYZ over the white -> Lab
__device__ __forceinline__ double cie_f(double t)
{
    return t > 216.0 / 24389.0 ? cie_cbrt(t) : (((24389.0 / 27.0) * t) + 16.0) / 116.0;
}
__device__ __forceinline__ cie_lab cie_lab_of(float fr, float fg, float fb)
{
    const double er = (double)fr, eg = (double)fg, eb = (double)fb;
    const double x = ((0.412453 * er) + (0.357580 * eg)) + (0.180423 * eb);
    const double y = ((0.212671 * er) + (0.715160 * eg)) + (0.072169 * eb);
    const double z = ((0.019334 * er) + (0.119193 * eg)) + (0.950227 * eb);
    const double fx = cie_f(x / 0.950456), fy = cie_f(y), fz = cie_f(z / 1.088754);
    cie_lab o;
    o.l = (116.0 * fy) - 16.0;
    o.a = 500.0 * (fx - fy);
    o.b = 200.0 * (fy - fz);
    return o;
}

// step 4 up to its last line: the lightness, chroma and hue terms dL / S_L, dC / S_C, dH / S_H of two Lab values, signed, and
// the rotation factor R_T - what cie_de2000_q20 finishes and what the maps (ciede2000_map_kernel.h) show term by term
struct cie_terms {
    double tl, tc, th, rt;
};
__device__ __forceinline__ cie_terms cie_de2000_terms(const cie_lab &p1, const cie_lab &p2)
{
    constexpr double k25_7 = 6103515625.0;
    const double c1 = __builtin_sqrt((p1.a * p1.a) + (p1.b * p1.b));
    const double c2 = __builtin_sqrt((p2.a * p2.a) + (p2.b * p2.b));
    const double cb = 0.5 * (c1 + c2);
    const double cb7 = cie_pow7(cb);
    const double g = 0.5 * (1.0 - __builtin_sqrt(cb7 / (cb7 + k25_7)));
    const double ap1 = (1.0 + g) * p1.a;
    const double ap2 = (1.0 + g) * p2.a;
    const double cp1 = __builtin_sqrt((ap1 * ap1) + (p1.b * p1.b));
    const double cp2 = __builtin_sqrt((ap2 * ap2) + (p2.b * p2.b));
    const double h1 = cie_hue_deg(p1.b, ap1);
    const double h2 = cie_hue_deg(p2.b, ap2);
    const double dl = p2.l - p1.l;
    const double dc = cp2 - cp1;
    const double cc = cp1 * cp2;
    const bool nz = cc != 0.0;
    double dh = h2 - h1;
    dh = dh > 180.0 ? dh - 360.0 : dh < -180.0 ? dh + 360.0 : dh;
    dh = nz ? dh : 0.0;
    const double dH = (2.0 * __builtin_sqrt(cc)) * cie_sin_deg(0.5 * dh);
    const double hs = h1 + h2, hd = h1 - h2;
    const double hb = !nz ? hs : (hd < 0.0 ? -hd : hd) <= 180.0 ? 0.5 * hs : hs < 360.0 ? 0.5 * (hs + 360.0) : 0.5 * (hs - 360.0);
    const double lb = 0.5 * (p1.l + p2.l);
    const double cpb = 0.5 * (cp1 + cp2);
    const double t = (((1.0 - (0.17 * cie_cos_deg(hb - 30.0))) + (0.24 * cie_cos_deg(2.0 * hb))) + (0.32 * cie_cos_deg((3.0 * hb) + 6.0))) -
                     (0.20 * cie_cos_deg((4.0 * hb) - 63.0));
    const double z = (hb - 275.0) / 25.0;
    const double dth = 30.0 * cie_exp(-(z * z));
    const double cpb7 = cie_pow7(cpb);
    const double rc = 2.0 * __builtin_sqrt(cpb7 / (cpb7 + k25_7));
    const double l50 = lb - 50.0;
    const double l50s = l50 * l50;
    const double sl = 1.0 + ((0.015 * l50s) / __builtin_sqrt(20.0 + l50s));
    const double sc = 1.0 + (0.045 * cpb);
    const double sh = 1.0 + ((0.015 * cpb) * t);
    const double rt = (-cie_sin_deg(2.0 * dth)) * rc;
    const double tl = dl / sl, tc = dc / sc, th = dH / sh;
    cie_terms o;
    o.tl = tl, o.tc = tc, o.th = th, o.rt = rt;
    return o;
}

// the last line of step 4 and step 5: the terms -> q = rint(dE 2^20)
__device__ __forceinline__ uint32_t cie_terms_q20(const cie_terms &e)
{
    const double tl = e.tl, tc = e.tc, th = e.th, rt = e.rt;
    const double s = (((tl * tl) + (tc * tc)) + (th * th)) + (rt * (tc * th));
    const double de = __builtin_sqrt(s > 0.0 ? s : 0.0);
    return (uint32_t)(unsigned long long)__builtin_rint(de * 1048576.0);
}

// steps 4 and 5: CIEDE2000 of two Lab values -> q
__device__ __forceinline__ uint32_t cie_de2000_q20(const cie_lab &p1, const cie_lab &p2)
{
    return cie_terms_q20(cie_de2000_terms(p1, p2));
}

// one pixel of a pair: the six table values of its two sides -> q
__device__ __forceinline__ uint32_t cie_pixel_q20(const float ref[3], const float test[3])
{
    return cie_de2000_q20(cie_lab_of(ref[0], ref[1], ref[2]), cie_lab_of(test[0], test[1], test[2]));
}

}  // namespace
