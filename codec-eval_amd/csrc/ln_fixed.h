// ln x for a normal x >= 1 as a fixed sequence of separately rounded f64 operations (include/ce_metrics.h: ce_yuv_plane_vif,
// "Logarithm"): the first half of hlg_pixel.h's hlg_pow, operation for operation, in a header of its own so that the VIF kernel
// (plane_vif_kernel.h) and a host build of it read one text.  x = m 2^e with m in [sqrt(1/2), sqrt(2)); ln m = 2 t P(t^2) with
// t = (m - 1) / (m + 1) and P the odd-reciprocal series to 1/21 in Horner form; ln x = ln m + e ln2.  The quotients of literals
// are folded by the compiler, correctly rounded.  Nothing but the HIP keywords: compiled with -ffp-contract=off on both sides.
#pragma once

#include <cstdint>

namespace {

__device__ __forceinline__ double ln_fixed(double x)
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
    return (2.0 * t) * p + (double)e * kLn2;
}

}  // namespace
