// The device code of PSNR-HVS / PSNR-HVS-M on a decoder's planes (plane_hvs.hip; include/ce_metrics.h: ce_yuv_plane_hvs;
// DESIGN.md section 32), kept like plane_fidelity_kernel.h free of anything but the HIP keywords and blockIdx / threadIdx, so
// that tests/cpp/plane_hvs_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  The
// planes and the sample rule are plane_fidelity_kernel.h's pf_plane / pf_sample.  Eight lanes share a DCT block, so a thread
// block of 256 takes 32 of them, in three phases that two barriers separate:
//   hvs_rows     lane r loads row r of the block on both sides through the plane table, transforms it and leaves the eight
//                values in LDS, with the row's integer sums (left and right half: sum z, sum z^2) beside them
//   hvs_columns  lane l transforms column l of both sides and keeps DA[.][l], DB[.][l]; it leaves the column's share of the
//                mask's energy, sum (D D) mc down the column, in LDS
//   hvs_score    every lane of the block forms the same two masks from the eight column sums and the integer sums, then
//                thresholds and quantises its own eight coefficients into two integers
// Nothing crosses lanes but through LDS, so the host build needs no stand-in for a shuffle; the reduction of the two integers
// across the thread block stays in plane_hvs.hip.  Every f64 operation is written out and separately rounded
// (-ffp-contract=off); the sums run in the order the header states.
#pragma once

#include "plane_fidelity_kernel.h"

namespace {

constexpr uint32_t kHvsThreads = 256, kHvsWaves = kHvsThreads / 64;
constexpr uint32_t kHvsBlocks = kHvsThreads / 8;  // DCT blocks a thread block
constexpr uint32_t kHvsRow = 9;                   // f64 words a row of a DCT block takes in LDS: eight and one of padding (odd: lanes r = 0 .. 7 hit distinct banks)
constexpr uint32_t kHvsOut = 3 * 2 * 2;           // u64 a pair: [plane][hvs, hvsm][low, high]

// g[0] = sqrt(1 / 8), g[m] = cos(m pi / 16) / 2 for m = 1 .. 7, each the nearest f64 (tests/test_plane_hvs_cpu.py checks them
// against 30 digits and against the restatement's text)
__device__ __forceinline__ constexpr double hvs_g(int m)
{
    return m == 0   ? 0x1.6a09e667f3bcdp-2
           : m == 1 ? 0x1.f6297cff75cb0p-2
           : m == 2 ? 0x1.d906bcf328d46p-2
           : m == 3 ? 0x1.a9b66290ea1a3p-2
           : m == 4 ? 0x1.6a09e667f3bcdp-2
           : m == 5 ? 0x1.1c73b39ae68c8p-2
           : m == 6 ? 0x1.87de2a6aea963p-3
                    : 0x1.8f8b83c69a60bp-4;
}

// T[k][j] of the orthonormal DCT-II: g[0] for k = 0, else cos((2j + 1) k pi / 16) / 2 = +-g[m], a = (2j + 1) k mod 32 folded by
// cos(2 pi - x) = cos x and cos(pi - x) = -cos x (a is never 0, 8, 16 or 24 for k = 1 .. 7).  k and j are constants wherever
// this is called, so it is a literal there.
__device__ __forceinline__ constexpr double hvs_t(int k, int j)
{
    if (k == 0) return hvs_g(0);
    int a = ((2 * j + 1) * k) % 32;
    if (a > 16) a = 32 - a;
    return a > 8 ? -hvs_g(16 - a) : hvs_g(a);
}

// out[k] = ((((((T[k][0] x0 + T[k][1] x1) + T[k][2] x2) + ...) + T[k][7] x7
__device__ __forceinline__ void hvs_dct8(const double (&x)[8], double (&out)[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double s = hvs_t(k, 0) * x[0] + hvs_t(k, 1) * x[1];
#pragma unroll
        for (int j = 2; j < 8; j++) s = s + hvs_t(k, j) * x[j];
        out[k] = s;
    }
}

struct hvs_args {
    const pf_plane *tab;        // [n_refs + n_pairs][3]: the references' planes, then the tests'
    const uint32_t *pair_ref;   // pair -> reference
    const double *csf, *mc;     // [8][8] each
    unsigned long long *out;    // [pair][kHvsOut]
    uint32_t n_refs, n_planes;  // blockIdx.y = (pair - first) * n_planes + plane
    uint32_t w[3], h[3];        // the planes' sizes
    uint32_t maxv, first, step;
    double unit;                // 2^(36 - 2d)
};

// what a thread block's LDS holds, per DCT block and side
struct hvs_lds {
    double d[kHvsBlocks][2][8][kHvsRow];  // the row-transformed block, [row][coefficient]
    double c[kHvsBlocks][2][8];           // column l's sum of (D D) mc
    uint32_t s[kHvsBlocks][2][8][4];      // row r's sum z over columns 0 - 3 and 4 - 7, then its sum z^2 alike (8 * 4095^2 < 2^32)
};

// the thread's pair, plane and DCT block; dead where the plane has fewer blocks than the grid's x covers (the grid is sized
// for luma)
struct hvs_where {
    uint32_t pair, plane, x, y;
    bool live;
};
__device__ __forceinline__ hvs_where hvs_block(const hvs_args &a)
{
    hvs_where o;
    o.pair = a.first + blockIdx.y / a.n_planes, o.plane = blockIdx.y % a.n_planes;
    const uint32_t pw = a.w[o.plane], ph = a.h[o.plane];
    const uint32_t nx = pw < 8 ? 0 : (pw - 8) / a.step + 1, ny = ph < 8 ? 0 : (ph - 8) / a.step + 1;
    const unsigned long long at = (unsigned long long)blockIdx.x * kHvsBlocks + threadIdx.x / 8u;
    o.live = at < (unsigned long long)nx * ny;
    o.x = o.live ? (uint32_t)(at % nx) * a.step : 0, o.y = o.live ? (uint32_t)(at / nx) * a.step : 0;
    return o;
}

template <class SAMPLE>
__device__ __forceinline__ void hvs_rows(const hvs_args &a, hvs_lds &lds)
{
    const hvs_where o = hvs_block(a);
    if (!o.live) return;
    const uint32_t r = threadIdx.x % 8u, b = threadIdx.x / 8u;
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const pf_plane pl = a.tab[(side ? (size_t)a.n_refs + o.pair : (size_t)a.pair_ref[o.pair]) * 3 + o.plane];
        double x[8], out[8];
        uint32_t sum[2] = {0, 0}, sq[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t z = pf_sample<SAMPLE>(pl, o.x + j, o.y + r, a.maxv);
            sum[j / 4] += z, sq[j / 4] += z * z;
            x[j] = (double)z;
        }
        hvs_dct8(x, out);
#pragma unroll
        for (int k = 0; k < 8; k++) lds.d[b][side][r][k] = out[k];
        lds.s[b][side][r][0] = sum[0], lds.s[b][side][r][1] = sum[1], lds.s[b][side][r][2] = sq[0], lds.s[b][side][r][3] = sq[1];
    }
}

// column l of the block's two sides, held from hvs_columns to hvs_score
struct hvs_cols {
    double d[2][8];
};

__device__ __forceinline__ void hvs_columns(const hvs_args &a, hvs_lds &lds, hvs_cols &col)
{
    const hvs_where o = hvs_block(a);
    if (!o.live) return;
    const uint32_t l = threadIdx.x % 8u, b = threadIdx.x / 8u;
#pragma unroll
    for (int side = 0; side < 2; side++) {
        double x[8];
#pragma unroll
        for (int r = 0; r < 8; r++) x[r] = lds.d[b][side][r][l];
        hvs_dct8(x, col.d[side]);
        // from k = 0 down, without the DC term: 0.0 + t is t, so column 0 starts at k = 1
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double t = (col.d[side][k] * col.d[side][k]) * a.mc[k * 8 + l];
            c = k == 0 ? (l == 0 ? 0.0 : t) : c + t;
        }
        lds.c[b][side][l] = c;
    }
}

// N sum z^2 - (sum z)^2
__device__ __forceinline__ unsigned long long hvs_spread(uint32_t n, unsigned long long sum, unsigned long long sq) { return n * sq - sum * sum; }

// the mask of one side of DCT block b, the same in all of its lanes
__device__ __forceinline__ double hvs_mask(const hvs_lds &lds, uint32_t b, int side)
{
    const double *c = lds.c[b][side];
    const double m = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
    unsigned long long sum[2][2] = {}, sq[2][2] = {};  // [rows 0 - 3, 4 - 7][columns 0 - 3, 4 - 7]
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t *s = lds.s[b][side][r];
        sum[r / 4][0] += s[0], sum[r / 4][1] += s[1], sq[r / 4][0] += s[2], sq[r / 4][1] += s[3];
    }
    const unsigned long long whole = hvs_spread(64, (sum[0][0] + sum[0][1]) + (sum[1][0] + sum[1][1]), (sq[0][0] + sq[0][1]) + (sq[1][0] + sq[1][1]));
    const unsigned long long quads = (hvs_spread(16, sum[0][0], sq[0][0]) + hvs_spread(16, sum[0][1], sq[0][1])) +
                                     (hvs_spread(16, sum[1][0], sq[1][0]) + hvs_spread(16, sum[1][1], sq[1][1]));
    const double pop = whole == 0 ? 0.0 : (63.0 * (double)quads) / (15.0 * (double)whole);
    return __builtin_sqrt(m * pop) / 32.0;
}

// q[0], q[1]: the thread's share of sum q_hvs and sum q_hvsm, its eight coefficients (0 in a dead thread)
__device__ __forceinline__ void hvs_score(const hvs_args &a, const hvs_lds &lds, const hvs_cols &col, unsigned long long (&q)[2])
{
    q[0] = q[1] = 0;
    const hvs_where o = hvs_block(a);
    if (!o.live) return;
    const uint32_t l = threadIdx.x % 8u, b = threadIdx.x / 8u;
    const double ma = hvs_mask(lds, b, 0), mb = hvs_mask(lds, b, 1);
    const double M = ma > mb ? ma : mb;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double u = __builtin_fabs(col.d[0][k] - col.d[1][k]);
        const double t = M / a.mc[k * 8 + l];
        const double um = (k == 0 && l == 0) ? u : u < t ? 0.0 : u - t;
        const double csf = a.csf[k * 8 + l];
        const double p = u * csf, pm = um * csf;
        q[0] += (unsigned long long)__builtin_rint((p * p) * a.unit);
        q[1] += (unsigned long long)__builtin_rint((pm * pm) * a.unit);
    }
}

}  // namespace
