// The device code of GMSD on a decoder's planes (plane_gmsd.hip; include/ce_metrics.h: ce_yuv_plane_gmsd),
// kept like plane_fidelity_kernel.h free of anything but the HIP keywords and blockIdx / threadIdx, so that
// tests/cpp/plane_gmsd_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  The planes
// and the sample rule are plane_fidelity_kernel.h's pf_plane / pf_sample, the wide loads its pf_wide_ok / pf_load16.  The
// definition was written from the paper's MATLAB code as remembered; nothing here was checked against that code itself.  A
// thread block takes a tile of kGmsdTileW x kGmsdTileH positions of one plane of one pair, in two phases that one barrier
// separates:
//   gmsd_stage  the 2 x 2 sums S of both sides as int32 in LDS, the tile's positions with a rim of one: a work item is 16
//               bytes of samples of a row pair (8 positions of u8, 4 of u16) where both rows admit the wide path and the piece
//               lies wholly in the row, the same positions sample by sample where not.  Zeros outside the grid, so the
//               gradient has no branch at an edge.
//   gmsd_score  a thread takes kGmsdRows positions of one column: the Prewitt sums from 6 x 3 values of S a side, A, g and q
//               per position, and its share of sum q, of the three partial second moments and of the largest 2^32 - q.
// Nothing crosses lanes but through LDS; the reduction across the thread block stays in plane_gmsd.hip.  Every f64 operation
// is written out and separately rounded (-ffp-contract=off).  gmsd_finish is the host's finishing, plain C++.
#pragma once

#include "plane_fidelity_kernel.h"

namespace {

constexpr uint32_t kGmsdTileW = 64, kGmsdTileH = 16;  // positions a thread block
constexpr uint32_t kGmsdThreads = 256, kGmsdWaves = kGmsdThreads / 64;
constexpr uint32_t kGmsdRows = kGmsdTileH / (kGmsdThreads / kGmsdTileW);  // positions a thread, down one column
constexpr uint32_t kGmsdSumW = kGmsdTileW + 2, kGmsdSumH = kGmsdTileH + 2;
constexpr uint32_t kGmsdTerms = 5;                // u64 a plane: sum q, sum qh qh, sum qh ql, sum ql ql, max (2^32 - q); q = qh 2^16 + ql
constexpr uint32_t kGmsdOut = 3 * kGmsdTerms;     // u64 a pair
static_assert(kGmsdThreads % kGmsdTileW == 0 && kGmsdTileH % (kGmsdThreads / kGmsdTileW) == 0, "a thread takes whole positions of one column");
static_assert(kGmsdTileW % 8 == 0, "a 16-byte piece of u8 samples is 8 positions and must not straddle a tile's first column");

struct gmsd_args {
    const pf_plane *tab;        // [n_refs + n_pairs][3]: the references' planes, then the tests'
    const uint32_t *pair_ref;   // pair -> reference
    unsigned long long *out;    // [pair][kGmsdOut]
    uint32_t n_refs, n_planes;  // blockIdx.y = (pair - first) * n_planes + plane
    uint32_t w[3], h[3];        // the planes' sizes in samples
    uint32_t maxv, first;
    unsigned long long k;       // 24480 * 4^(d - 8)
};

// what a thread block's LDS holds: S of [reference, test] at positions (x0 - 1 .. x0 + TW, y0 - 1 .. y0 + TH)
struct gmsd_lds {
    int32_t s[2][kGmsdSumH][kGmsdSumW];
};

// the block's pair, plane, grid of positions and tile origin; dead where the plane has fewer tiles than the grid's x covers
// (the grid is sized for luma)
struct gmsd_where {
    uint32_t pair, plane, w2, h2, x0, y0;
    bool live;
};
__device__ __forceinline__ gmsd_where gmsd_tile(const gmsd_args &a)
{
    gmsd_where o;
    o.pair = a.first + blockIdx.y / a.n_planes, o.plane = blockIdx.y % a.n_planes;
    o.w2 = a.w[o.plane] / 2u + (a.w[o.plane] & 1u), o.h2 = a.h[o.plane] / 2u + (a.h[o.plane] & 1u);
    const uint32_t tiles_x = (o.w2 + kGmsdTileW - 1) / kGmsdTileW, tiles_y = (o.h2 + kGmsdTileH - 1) / kGmsdTileH;
    o.live = blockIdx.x < (unsigned long long)tiles_x * tiles_y;
    o.x0 = o.live ? (blockIdx.x % tiles_x) * kGmsdTileW : 0, o.y0 = o.live ? (blockIdx.x / tiles_x) * kGmsdTileH : 0;
    return o;
}

// v[k] += the two samples 2k, 2k + 1 of 16 bytes of a row as pf_load16 returns them; u8 has neither shift nor clamp (pf_sse16)
template <int BPS>
__device__ __forceinline__ void gmsd_add16(const uint4 u, uint32_t shift, uint32_t maxv, int32_t (&v)[8 / BPS])
{
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
        if constexpr (BPS == 1) {
            v[2 * d] += (int32_t)((w[d] & 0xffu) + ((w[d] >> 8) & 0xffu));
            v[2 * d + 1] += (int32_t)(((w[d] >> 16) & 0xffu) + (w[d] >> 24));
        } else {
            uint32_t lo = (w[d] & 0xffffu) >> shift, hi = (w[d] >> 16) >> shift;
            lo = lo < maxv ? lo : maxv, hi = hi < maxv ? hi : maxv;
            v[d] += (int32_t)(lo + hi);
        }
    }
}

template <class SAMPLE>
__device__ __forceinline__ void gmsd_stage(const gmsd_args &a, gmsd_lds &lds)
{
    constexpr int BPS = sizeof(SAMPLE);
    constexpr uint32_t N = 16 / BPS, G = N / 2;    // samples and positions in 16 bytes
    constexpr uint32_t kPieces = kGmsdTileW / G + 2;  // pieces aligned to G positions that cover x0 - 1 .. x0 + TW: x0 is a multiple of G
    const gmsd_where o = gmsd_tile(a);
    if (!o.live) return;
    const uint32_t pw = a.w[o.plane], ph = a.h[o.plane];
    for (uint32_t item = threadIdx.x; item < 2 * kGmsdSumH * kPieces; item += kGmsdThreads) {
        const uint32_t side = item / (kGmsdSumH * kPieces), r = item / kPieces % kGmsdSumH, g = item % kPieces;
        // row j of S and the piece's first position, before the grid where negative
        const long long j = (long long)o.y0 + r - 1, i0 = (long long)o.x0 + ((long long)g - 1) * G;
        int32_t v[G];
#pragma unroll
        for (uint32_t k = 0; k < G; k++) v[k] = 0;
        if (j >= 0 && j < (long long)o.h2 && i0 >= 0 && i0 < (long long)o.w2) {
            const pf_plane pl = a.tab[(side ? (size_t)a.n_refs + o.pair : (size_t)a.pair_ref[o.pair]) * 3 + o.plane];
            const uint32_t y = 2u * (uint32_t)j;      // y < ph; the row under it may be outside
            const bool two = y + 1u < ph;
            const uint8_t *row0 = pl.base + (size_t)y * pl.pitch, *row1 = row0 + (two ? pl.pitch : 0);
            const size_t piece = (size_t)(i0 / G);
            if (piece < pw / N && pf_wide_ok<BPS>(row0, pl.step, o.plane) && pf_wide_ok<BPS>(row1, pl.step, o.plane)) {
                gmsd_add16<BPS>(pf_load16<BPS>(row0, pl.step, piece), pl.shift, a.maxv, v);
                if (two) gmsd_add16<BPS>(pf_load16<BPS>(row1, pl.step, piece), pl.shift, a.maxv, v);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < G; k++) {
                    const unsigned long long x = 2ull * (unsigned long long)(i0 + k);
                    if (x < pw) v[k] += (int32_t)pf_sample<SAMPLE>(pl, (uint32_t)x, y, a.maxv);
                    if (x + 1 < pw) v[k] += (int32_t)pf_sample<SAMPLE>(pl, (uint32_t)x + 1u, y, a.maxv);
                    if (two && x < pw) v[k] += (int32_t)pf_sample<SAMPLE>(pl, (uint32_t)x, y + 1u, a.maxv);
                    if (two && x + 1 < pw) v[k] += (int32_t)pf_sample<SAMPLE>(pl, (uint32_t)x + 1u, y + 1u, a.maxv);
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < G; k++) {
            const int c = (int)(g * G + k) - (int)G + 1;  // position i0 + k sits in column i0 + k - (x0 - 1)
            if (c >= 0 && c < (int)kGmsdSumW) lds.s[side][r][c] = v[k];
        }
    }
}

// q of one position from the two sides' exact squared gradient magnitudes: five separately rounded f64 operations
__device__ __forceinline__ unsigned long long gmsd_q(unsigned long long a_ref, unsigned long long a_test, unsigned long long k)
{
    const double m_ref = __builtin_sqrt((double)a_ref), m_test = __builtin_sqrt((double)a_test);
    const double num = (2.0 * (m_ref * m_test)) + (double)k;  // 2.0 * x is exact
    const double den = (double)(a_ref + a_test + k);
    const double g = num / den;
    return (unsigned long long)__builtin_rint(g * 4294967296.0);
}

// a thread's, a wave's or a thread block's share of a plane of a pair
struct gmsd_part {
    unsigned long long q, hh, hl, ll;  // sum q, sum qh qh, sum qh ql, sum ql ql
    unsigned long long max_dis;
};

__device__ __forceinline__ gmsd_part gmsd_score(const gmsd_args &a, const gmsd_lds &lds)
{
    gmsd_part t{};
    const gmsd_where o = gmsd_tile(a);
    if (!o.live) return t;
    const uint32_t cx = threadIdx.x % kGmsdTileW, ry = threadIdx.x / kGmsdTileW * kGmsdRows;
    if (o.x0 + cx >= o.w2) return t;
    // per side and row of S the sum of the three columns (Gy) and the left column less the right (Gx)
    int32_t sum[2][kGmsdRows + 2], dif[2][kGmsdRows + 2];
#pragma unroll
    for (int side = 0; side < 2; side++)
#pragma unroll
        for (uint32_t r = 0; r < kGmsdRows + 2; r++) {
            const int32_t *s = &lds.s[side][ry + r][cx];
            sum[side][r] = (s[0] + s[1]) + s[2], dif[side][r] = s[0] - s[2];
        }
#pragma unroll
    for (uint32_t k = 0; k < kGmsdRows; k++) {
        if (o.y0 + ry + k >= o.h2) break;
        unsigned long long A[2];
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const long long gx = (dif[side][k] + dif[side][k + 1]) + dif[side][k + 2], gy = sum[side][k] - sum[side][k + 2];
            A[side] = (unsigned long long)(gx * gx) + (unsigned long long)(gy * gy);
        }
        const unsigned long long q = gmsd_q(A[0], A[1], a.k), qh = q >> 16, ql = q & 0xffffull;  // qh <= 2^16
        const unsigned long long dis = 4294967296ull - q;
        t.q += q, t.hh += qh * qh, t.hl += qh * ql, t.ll += ql * ql;
        t.max_dis = dis > t.max_dis ? dis : t.max_dis;
    }
    return t;
}

// ---- the host's finishing ---------------------------------------------------------------------------------------------------------

struct gmsd_plane_result {
    uint64_t sum_q, sum_q2[2], n_pos;
    double gmsd, gmsm;
    uint32_t max_dis;
};

// acc: the plane's kGmsdTerms accumulators as the thread blocks left them
inline gmsd_plane_result gmsd_finish(const unsigned long long *acc, uint32_t pw, uint32_t ph)
{
    gmsd_plane_result o{};
    const uint64_t n = (uint64_t)(pw / 2u + (pw & 1u)) * (ph / 2u + (ph & 1u));  // under 2^32: the call refuses more
    const unsigned __int128 q2 = ((unsigned __int128)acc[1] << 32) + ((unsigned __int128)acc[2] << 17) + acc[3];
    o.sum_q = acc[0], o.sum_q2[0] = (uint64_t)q2, o.sum_q2[1] = (uint64_t)(q2 >> 64), o.n_pos = n, o.max_dis = (uint32_t)acc[4];
    const unsigned __int128 v = (unsigned __int128)n * q2 - (unsigned __int128)acc[0] * acc[0];  // n sum q^2 >= (sum q)^2
    // the nearest double of v, ties to even, whatever the runtime's conversion does: the top 64 bits with a sticky bit
    // convert with one rounding, and the scaling by a power of two is exact
    int up = 0;
    for (unsigned __int128 t = v >> 64; t; t >>= 1) up++;
    double vd;
    if (up == 0) vd = (double)(uint64_t)v;
    else {
        const unsigned __int128 low = v & (((unsigned __int128)1 << up) - 1);
        const uint64_t top = (uint64_t)(v >> up) | (low != 0 ? 1u : 0u);  // bit 63 is set: bit 0 is far below the rounding position
        vd = __builtin_ldexp((double)top, up);
    }
    const double scale = (double)n * 4294967296.0;
    o.gmsd = __builtin_sqrt(vd) / scale, o.gmsm = (double)acc[0] / scale;
    return o;
}

}  // namespace
