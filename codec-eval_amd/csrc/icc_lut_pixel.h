// One pixel of the LUT-based ICC ingest (include/ce_metrics.h: the LUT definition, steps 1 to 6): icc_pixel.h's three table
// gathers, then the CLUT - a node is 16 bytes, one load; four of them for the tetrahedral interpolation, eight for the
// trilinear - the post-CLUT curves, the 3 x 4 matrix, the PCS decode, cicp_pixel.h's matrix (here f32(inv(A))) and its clamp.
// icc_lut_px is the pixel the frames take (cicp_kernel.h: k_tagged for linear slots; icc_kernel.h: k_icc_encode for u8 and u16
// slots).  Which stages a profile has and what kind each curve is are arguments, the same for every pixel of a launch: the
// branches on them are uniform, and the only template axis is the interpolation.  Curves and fractions stay in named scalars
// and fully unrolled loops of constant index, so nothing is indexed dynamically.  Host-compilable like the headers that
// include it, and compiled with -ffp-contract=off, which holds for the f64 of the power curves too.
#pragma once

#include "hlg_pixel.h"

namespace {

// a CLUT node on the device: three channels and padding
struct alignas(16) icc_lut_node {
    float x, y, z, w;
};

// a post-CLUT curve (ce_icc_lut_curve with its samples' address)
struct icc_lut_curve {
    const float *s;  // SAMPLED: n samples
    uint32_t kind;   // CE_ICC_LUT_CURVE_*
    uint32_t n;      // SAMPLED: the count; POWER: the para function type
    double q[7];     // POWER: g a b c d e f
};

enum { kIccPcsXyz = 0, kIccPcsLab = 1, kIccPcsLabLegacy = 2 };

struct icc_lut_args {
    cicp_args c;             // table: the red channel's input table, maxv + 1 entries; m: f32(inv(A))
    const float *table_g;    // maxv + 1 entries each
    const float *table_b;
    const icc_lut_node *clut;  // null: no CLUT
    uint32_t s0, s1;         // node strides of the first and the second axis (the third's is 1)
    uint32_t i0, i1, i2;     // g - 2 per axis
    float g0, g1, g2;        // f32(g - 1) per axis
    uint32_t has_m, has_b;   // whether any curve of the stage is not the identity
    uint32_t has_matrix;
    uint32_t pcs;            // kIccPcs*
    float mat[12];           // 3 x 3 row-major, then the offsets
    icc_lut_curve mc[3], bc[3];
};

__device__ __forceinline__ float icc_clip01f(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ double icc_clip01d(double x) { return !(x > 0.0) ? 0.0 : (x > 1.0 ? 1.0 : x); }

// B^g by the header's rules: B <= 0 or subnormal is 0; 0^g; the range rule on the exponent bits; else hlg_pow
__device__ __forceinline__ double icc_pow(double base, double g)
{
    if (!(base >= 2.2250738585072014e-308)) return g < 0.0 ? __builtin_inf() : (g == 0.0 ? 1.0 : 0.0);
    uint64_t bits;
    __builtin_memcpy(&bits, &base, 8);
    const int64_t e = (int64_t)((bits >> 52) & 0x7ffu) - 1023;
    const double ae = (double)(e < 0 ? -e : e);
    const double ag = g < 0.0 ? -g : g;
    if (ag * (ae + 1.0) > 1000.0) return g * ((double)e + 0.5) > 0.0 ? __builtin_inf() : 0.0;
    return hlg_pow(base, g);
}

// a POWER curve on the clipped x: the para formulas in f64 (curv n = 1 is type 0), clipped and rounded once
__device__ __forceinline__ float icc_power_curve(const icc_lut_curve &k, float xf)
{
    const double x = (double)xf;
    const double g = k.q[0], a = k.q[1], b = k.q[2], c = k.q[3], d = k.q[4], e = k.q[5], f = k.q[6];
    double y;
    if (k.n == 0) {
        y = icc_pow(x, g);
    } else {
        const double ax = a * x;
        const double p = icc_pow(ax + b, g);
        if (k.n == 1) y = x >= -b / a ? p : 0.0;
        else if (k.n == 2) y = x >= -b / a ? p + c : c;
        else if (k.n == 3) y = x >= d ? p : c * x;
        else {
            const double cx = c * x;
            y = x >= d ? p + e : cx + f;
        }
    }
    return (float)icc_clip01d(y);
}

// a SAMPLED curve on the clipped x
__device__ __forceinline__ float icc_sampled_curve(const icc_lut_curve &k, float x)
{
    const float p = x * (float)(k.n - 1);
    uint32_t i = (uint32_t)p;  // p in [0, n - 1]
    i = i < k.n - 2 ? i : k.n - 2;
    const float s0 = k.s[i], s1 = k.s[i + 1];
    const float fr = p - (float)i;
    const float d = s1 - s0;
    const float t = d * fr;
    return s0 + t;
}

__device__ __forceinline__ float icc_lut_curve_at(const icc_lut_curve &k, float x)
{
    if (k.kind == CE_ICC_LUT_CURVE_IDENTITY) return x;
    const float xc = icc_clip01f(x);
    return k.kind == CE_ICC_LUT_CURVE_SAMPLED ? icc_sampled_curve(k, xc) : icc_power_curve(k, xc);
}

// an axis of the CLUT: p = a * (g - 1), the cell and the fraction
__device__ __forceinline__ void icc_lut_axis(float a, float gm1, uint32_t imax, uint32_t &i, float &f)
{
    const float p = a * gm1;
    i = (uint32_t)p;  // a in [0, 1]: p in [0, g - 1]
    i = i < imax ? i : imax;
    f = p - (float)i;
}

__device__ __forceinline__ float icc_lerp(float c0, float c1, float f)
{
    const float d = c1 - c0;
    const float t = d * f;
    return c0 + t;
}

// Lab's cube / linear branch
__device__ __forceinline__ float icc_lab_t(float f)
{
    constexpr float k6_29 = (float)(6.0 / 29.0), k4_29 = (float)(4.0 / 29.0), k108_841 = (float)(108.0 / 841.0);
    const float f2 = f * f;
    const float cube = f2 * f;
    const float lin = (f - k4_29) * k108_841;
    return f > k6_29 ? cube : lin;
}

template <bool TETRA>
struct icc_lut_px {
    icc_lut_args a;
    __device__ __forceinline__ const cicp_args &frame() const { return a.c; }
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t g, uint32_t b, float (&o)[3]) const
    {
        const uint32_t m = a.c.maxv;
        float v0 = a.c.table[r < m ? r : m], v1 = a.table_g[g < m ? g : m], v2 = a.table_b[b < m ? b : m];
        if (a.clut) {
            uint32_t ix, iy, iz;
            float fx, fy, fz;
            icc_lut_axis(v0, a.g0, a.i0, ix, fx);
            icc_lut_axis(v1, a.g1, a.i1, iy, fy);
            icc_lut_axis(v2, a.g2, a.i2, iz, fz);
            const icc_lut_node *n = a.clut + ((size_t)ix * a.s0 + (size_t)iy * a.s1 + iz);
            if constexpr (TETRA) {
                // the axis of the largest fraction, then of the middle one: strides and fractions chosen by selects
                const bool xy = fx >= fy, yz = fy >= fz, xz = fx >= fz;
                uint32_t sh, sm;
                float hi, mid, lo;
                if (xy) {
                    if (yz) sh = a.s0, sm = a.s1, hi = fx, mid = fy, lo = fz;
                    else if (xz) sh = a.s0, sm = 1u, hi = fx, mid = fz, lo = fy;
                    else sh = 1u, sm = a.s0, hi = fz, mid = fx, lo = fy;
                } else {
                    if (xz) sh = a.s1, sm = a.s0, hi = fy, mid = fx, lo = fz;
                    else if (yz) sh = a.s1, sm = 1u, hi = fy, mid = fz, lo = fx;
                    else sh = 1u, sm = a.s1, hi = fz, mid = fy, lo = fx;
                }
                const icc_lut_node c000 = n[0], ca = n[sh], cb = n[(size_t)sh + sm], c111 = n[(size_t)a.s0 + a.s1 + 1u];
                {
                    const float d0 = ca.x - c000.x, d1 = cb.x - ca.x, d2 = c111.x - cb.x;
                    const float t0 = d0 * hi, t1 = d1 * mid, t2 = d2 * lo;
                    const float s0 = c000.x + t0;
                    const float s1 = s0 + t1;
                    v0 = s1 + t2;
                }
                {
                    const float d0 = ca.y - c000.y, d1 = cb.y - ca.y, d2 = c111.y - cb.y;
                    const float t0 = d0 * hi, t1 = d1 * mid, t2 = d2 * lo;
                    const float s0 = c000.y + t0;
                    const float s1 = s0 + t1;
                    v1 = s1 + t2;
                }
                {
                    const float d0 = ca.z - c000.z, d1 = cb.z - ca.z, d2 = c111.z - cb.z;
                    const float t0 = d0 * hi, t1 = d1 * mid, t2 = d2 * lo;
                    const float s0 = c000.z + t0;
                    const float s1 = s0 + t1;
                    v2 = s1 + t2;
                }
            } else {
                const size_t sx = a.s0, sy = a.s1;
                const icc_lut_node c000 = n[0], c001 = n[1], c010 = n[sy], c011 = n[sy + 1];
                const icc_lut_node c100 = n[sx], c101 = n[sx + 1], c110 = n[sx + sy], c111 = n[sx + sy + 1];
                v0 = icc_lerp(icc_lerp(icc_lerp(c000.x, c001.x, fz), icc_lerp(c010.x, c011.x, fz), fy),
                              icc_lerp(icc_lerp(c100.x, c101.x, fz), icc_lerp(c110.x, c111.x, fz), fy), fx);
                v1 = icc_lerp(icc_lerp(icc_lerp(c000.y, c001.y, fz), icc_lerp(c010.y, c011.y, fz), fy),
                              icc_lerp(icc_lerp(c100.y, c101.y, fz), icc_lerp(c110.y, c111.y, fz), fy), fx);
                v2 = icc_lerp(icc_lerp(icc_lerp(c000.z, c001.z, fz), icc_lerp(c010.z, c011.z, fz), fy),
                              icc_lerp(icc_lerp(c100.z, c101.z, fz), icc_lerp(c110.z, c111.z, fz), fy), fx);
            }
        }
        if (a.has_m) v0 = icc_lut_curve_at(a.mc[0], v0), v1 = icc_lut_curve_at(a.mc[1], v1), v2 = icc_lut_curve_at(a.mc[2], v2);
        if (a.has_matrix) {
            float y[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p0 = a.mat[3 * i] * v0, p1 = a.mat[3 * i + 1] * v1, p2 = a.mat[3 * i + 2] * v2;
                const float s01 = p0 + p1;
                const float s012 = s01 + p2;
                y[i] = s012 + a.mat[9 + i];
            }
            v0 = y[0], v1 = y[1], v2 = y[2];
        }
        if (a.has_b) v0 = icc_lut_curve_at(a.bc[0], v0), v1 = icc_lut_curve_at(a.bc[1], v1), v2 = icc_lut_curve_at(a.bc[2], v2);
        float X, Y, Z;
        if (a.pcs == kIccPcsXyz) {
            constexpr float kScale = 1.0f + 32767.0f / 32768.0f;
            X = v0 * kScale, Y = v1 * kScale, Z = v2 * kScale;
        } else {
            const bool legacy = a.pcs == kIccPcsLabLegacy;
            const float kl = legacy ? (float)(65535.0 / 652.8) : 100.0f, kab = legacy ? (float)(65535.0 / 256.0) : 255.0f;
            const float L = v0 * kl;
            const float pa = v1 * kab, pb = v2 * kab;
            const float la = pa - 128.0f, lb = pb - 128.0f;
            const float l16 = L + 16.0f;
            const float fy = l16 / 116.0f;
            const float qa = la / 500.0f, qb = lb / 200.0f;
            const float fx = fy + qa, fz = fy - qb;
            constexpr float kXw = (float)(0xF6D6 / 65536.0), kZw = (float)(0xD32D / 65536.0);
            X = kXw * icc_lab_t(fx), Y = icc_lab_t(fy), Z = kZw * icc_lab_t(fz);
        }
        cicp_matrix_clamp<true>(a.c, X, Y, Z, o);
    }
};

}  // namespace
