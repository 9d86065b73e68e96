// The device code of SSIM / MS-SSIM (msssim.hip; include/ce_metrics.h: ce_batch_msssim), kept like
// hdr_fidelity_kernel.h free of anything but the HIP keywords and blockIdx / threadIdx / gridDim, so that
// tests/cpp/msssim_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  The level
// kernel is split at its two barriers for that: mss_stage fills the LDS tile of the two planes, mss_columns filters the five
// streams down the columns into LDS, mss_lane filters them along the rows (mss_rows) and returns the lane's two integers, the
// sums of its positions' values (mss_position); the reduction across lanes stays in msssim.hip.  The map kernel
// (msssim_map_kernel.h) calls mss_rows and mss_position itself.  mss_pool_sample is the pooling kernel's one output sample.
//
// The arithmetic is f64 throughout, every product, sum and quotient rounded separately - this text is compiled with
// -ffp-contract=off on the device and on the host - and integers from the quantisation on.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

constexpr uint32_t kMssThreads = 256;
constexpr int kMssTaps = 11, kMssHalo = kMssTaps - 1;
constexpr int kMssTileW = 32, kMssTileH = 16;  // a block's outputs: T x U; a lane takes two neighbours of a row
constexpr int kMssInW = kMssTileW + kMssHalo, kMssInH = kMssTileH + kMssHalo;  // 42 x 26 samples a plane
constexpr int kMssInLen = kMssInW * kMssInH;       // floats a plane in LDS
constexpr int kMssColLen = kMssInW * kMssTileH;    // column-filtered values a stream: 42 (an even pitch) x 16 doubles
constexpr int kMssStreams = 5;                     // x, y, x*x, y*y, x*y
static_assert(kMssThreads == (kMssTileW / 2) * kMssTileH, "one lane per two outputs");
static_assert(kMssInW % 2 == 0, "rows of the column-filtered streams start 16-byte aligned");

// ce_msssim_window's literals: exp(-(i - 5)^2 / 4.5) over their sum, as numpy gives them
constexpr double kMssG[6] = {0.00102838008447911, 0.007598758135239185, 0.03600077212843083,
                             0.10936068950970002, 0.2130055377112537,   0.26601172486179436};
constexpr double mss_g(int i) { return kMssG[i < 6 ? i : 10 - i]; }  // constexpr: the device code and ce_msssim_window read it

struct alignas(16) mss_d2 {
    double a, b;
};

// One level of pairs [first, ...): the planes of the two sides as SAMPLE elements.  Level 0 reads the slabs (packed RGB:
// px = 3, chan = 1), the others the planar pyramid (px = 1, chan = w * h).
struct mss_args {
    const void *refs, *tests;      // slot 0 of either side at this level
    size_t ref_slot, test_slot;    // elements from a slot to the next
    size_t chan, px;               // elements from a channel to the next, from a sample to its right neighbour
    const uint32_t *pair_ref;      // pair -> reference slot
    uint32_t w, h;                 // the level's planes, both >= 11
    uint32_t tiles_x;              // tiles a row of tiles: ceil((w - 10) / T)
    uint32_t first, level;
    double c1, c2;
};

// the block's pair, channel and tile origin
struct mss_where {
    uint32_t pair, c, x0, y0;
};
__device__ __forceinline__ mss_where mss_block(const mss_args &a)
{
    mss_where o;
    o.pair = a.first + blockIdx.y / 3u, o.c = blockIdx.y % 3u;
    o.x0 = (blockIdx.x % a.tiles_x) * kMssTileW, o.y0 = (blockIdx.x / a.tiles_x) * kMssTileH;
    return o;
}

// Before the first barrier: the tile of the two planes with its halo, zeros outside the plane (those feed masked outputs only).
template <class SAMPLE>
__device__ __forceinline__ void mss_stage(const mss_args &a, float *s_in)
{
    const mss_where o = mss_block(a);
    const SAMPLE *x = static_cast<const SAMPLE *>(a.refs) + (size_t)a.pair_ref[o.pair] * a.ref_slot + (size_t)o.c * a.chan;
    const SAMPLE *y = static_cast<const SAMPLE *>(a.tests) + (size_t)o.pair * a.test_slot + (size_t)o.c * a.chan;
    for (int i = threadIdx.x; i < kMssInLen; i += kMssThreads) {
        const uint32_t gy = o.y0 + i / kMssInW, gx = o.x0 + i % kMssInW;
        const bool in = gy < a.h && gx < a.w;
        const size_t at = ((size_t)gy * a.w + gx) * a.px;
        s_in[i] = in ? (float)x[at] : 0.0f;
        s_in[kMssInLen + i] = in ? (float)y[at] : 0.0f;
    }
}

// Between the barriers: v[stream][r][c] = sum_i g[i] * p[r + i][c] for the five streams, U x (T + 10) values each.
__device__ __forceinline__ void mss_columns(const float *s_in, double *s_col)
{
    for (int j = threadIdx.x; j < kMssColLen; j += kMssThreads) {
        double v[kMssStreams] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < kMssTaps; i++) {
            const double x = (double)s_in[j + i * kMssInW], y = (double)s_in[kMssInLen + j + i * kMssInW], g = mss_g(i);
            v[0] = v[0] + g * x;
            v[1] = v[1] + g * y;
            v[2] = v[2] + g * (x * x);
            v[3] = v[3] + g * (y * y);
            v[4] = v[4] + g * (x * y);
        }
#pragma unroll
        for (int k = 0; k < kMssStreams; k++) s_col[k * kMssColLen + j] = v[k];
    }
}

// s and cs of one position from the five filtered values, quantised: q[0] = qs, q[1] = qc.  The one text of a position's
// values: the scores sum it (mss_quantise), the maps store it (msssim_map_kernel.h).
__device__ __forceinline__ void mss_position(const mss_args &a, const double f[kMssStreams], long long q[2])
{
    const double mx = f[0], my = f[1];
    const double sxx = f[2] - mx * mx, syy = f[3] - my * my, sxy = f[4] - mx * my;
    const double cs = (2.0 * sxy + a.c2) / ((sxx + syy) + a.c2);
    const double lum = (2.0 * (mx * my) + a.c1) / ((mx * mx + my * my) + a.c1);
    const double s = lum * cs;
    q[0] = (long long)__builtin_rint(s * 4294967296.0);
    q[1] = (long long)__builtin_rint(cs * 4294967296.0);
}

// ... added to the lane's sums
__device__ __forceinline__ void mss_quantise(const mss_args &a, const double f[kMssStreams], long long acc[2])
{
    long long q[2];
    mss_position(a, f, q);
    acc[0] += q[0];
    acc[1] += q[1];
}

// After the second barrier: the five streams filtered along the rows for the lane's two outputs, neighbours of one row -
// twelve values of each stream, read as six 16-byte pairs.
__device__ __forceinline__ void mss_rows(const double *s_col, double f0[kMssStreams], double f1[kMssStreams])
{
    const int lx = (threadIdx.x % (kMssTileW / 2)) * 2, ly = threadIdx.x / (kMssTileW / 2);
#pragma unroll
    for (int k = 0; k < kMssStreams; k++) {
        const mss_d2 *row = reinterpret_cast<const mss_d2 *>(s_col + k * kMssColLen + ly * kMssInW + lx);
        double v[kMssTaps + 1];
#pragma unroll
        for (int i = 0; i < (kMssTaps + 1) / 2; i++) {
            const mss_d2 d = row[i];
            v[2 * i] = d.a, v[2 * i + 1] = d.b;
        }
        double o0 = 0.0, o1 = 0.0;
#pragma unroll
        for (int i = 0; i < kMssTaps; i++) {
            o0 = o0 + mss_g(i) * v[i];
            o1 = o1 + mss_g(i) * v[i + 1];
        }
        f0[k] = o0, f1[k] = o1;
    }
}

// ... and the lane's two integers: acc = sum of qs, sum of qc over those of its two outputs that lie in the plane's valid region.
__device__ __forceinline__ void mss_lane(const mss_args &a, const double *s_col, long long acc[2])
{
    const mss_where o = mss_block(a);
    const int lx = (threadIdx.x % (kMssTileW / 2)) * 2, ly = threadIdx.x / (kMssTileW / 2);
    double f0[kMssStreams], f1[kMssStreams];
    mss_rows(s_col, f0, f1);
    acc[0] = acc[1] = 0;
    const uint32_t vw = a.w - kMssHalo, vh = a.h - kMssHalo, gx = o.x0 + lx, gy = o.y0 + ly;
    if (gy < vh && gx < vw) mss_quantise(a, f0, acc);
    if (gy < vh && gx + 1 < vw) mss_quantise(a, f1, acc);
}

// One level of slots [first, ...) of one side pooled into the next: src as mss_args describes a level, dst planar f32.
struct mss_pool_args {
    const void *src;
    float *dst;
    size_t src_slot, dst_slot;  // elements from a slot to the next
    size_t chan, px;            // of src
    uint32_t w, h;              // src planes
    uint32_t ow, oh;            // dst planes: (w + (w & 1)) / 2, (h + (h & 1)) / 2
    uint32_t first;
};

// dst sample `i` of [3][oh][ow] of slot first + blockIdx.y: the mean of the 2 x 2 samples of src padded with h & 1 rows of
// zeros above and w & 1 columns on the left.  The sums are exact in f64 (and the result in f32).
template <class SAMPLE>
__device__ __forceinline__ void mss_pool_sample(const mss_pool_args &a, size_t i)
{
    const uint32_t slot = a.first + blockIdx.y;
    const size_t plane = (size_t)a.ow * a.oh;
    const uint32_t c = (uint32_t)(i / plane), Y = (uint32_t)((i % plane) / a.ow), X = (uint32_t)(i % a.ow);
    const SAMPLE *p = static_cast<const SAMPLE *>(a.src) + (size_t)slot * a.src_slot + (size_t)c * a.chan;
    const uint32_t pw = a.w & 1u, ph = a.h & 1u;
    double q[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const uint32_t qy = 2 * Y + dy, qx = 2 * X + dx;  // in the padded plane
            q[dy][dx] = (qy >= ph && qx >= pw) ? (double)p[((size_t)(qy - ph) * a.w + (qx - pw)) * a.px] : 0.0;
        }
    a.dst[(size_t)slot * a.dst_slot + i] = (float)(((q[0][0] + q[0][1]) + (q[1][0] + q[1][1])) * 0.25);
}

}  // namespace
