// The device code of pixel-domain VIF on a decoder's planes (plane_vif.hip; include/ce_metrics.h: ce_yuv_plane_vif; DESIGN.md
// section 33), kept like plane_hvs_kernel.h free of anything but the HIP keywords and blockIdx / threadIdx, so that
// tests/cpp/plane_vif_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  The planes
// and the sample rule are plane_fidelity_kernel.h's pf_plane / pf_sample; the shape is msssim_kernel.h's level kernel with the
// window length N as a template parameter (17, 9, 5, 3 for scales 1 - 4).  The stats kernel of one scale is split at its two
// barriers:
//   vif_stage     the T x U tile of the two sides with its N - 1 halo into LDS, zeros outside the plane (those feed masked
//                 outputs only): scale 1 from the plane table as u8 / u16 times 2^(8 - d), held as f32 (at most 12 significant
//                 bits: exact), scales 2 - 4 from the f64 pyramid
//   vif_columns   the five streams x, y, x * x, y * y, x * y filtered down the columns into LDS
//   vif_lane      ... filtered along the rows for the lane's four outputs, two neighbours in each of two rows, then the
//                 per-position text (vif_position) and the lane's two integers
// The reduction of the two integers across the thread block stays in plane_vif.hip.  The reduce kernel, which writes the next
// scale - F_s of the previous one at its even rows and even columns - has the same three phases on a 16 x 16 tile of outputs:
// vif_reduce_stage, vif_reduce_columns (the even rows only), vif_reduce_rows (one output a lane).  Every f64 operation is written out
// and separately rounded (-ffp-contract=off); the sums run in the order the header states.
#pragma once

#include <type_traits>

#include "plane_fidelity_kernel.h"

#include "ln_fixed.h"

namespace {

constexpr uint32_t kVifThreads = 256, kVifWaves = kVifThreads / 64;
constexpr int kVifScales = 4;
constexpr int kVifTileW = 32, kVifTileH = 32;  // a block's outputs: T x U; a lane takes two neighbours of a row, in two rows U / 2 apart
constexpr int kVifStreams = 5;                 // x, y, x*x, y*y, x*y
constexpr uint32_t kVifOut = 3 * kVifScales * 2;  // u64 a pair: [plane][scale][num, den]
static_assert(kVifThreads == (kVifTileW / 2) * (kVifTileH / 2), "one lane per four outputs");

constexpr int vif_taps(int scale) { return scale == 0 ? 17 : scale == 1 ? 9 : scale == 2 ? 5 : 3; }  // scale 0 .. 3 here

// ce_vif_window's literals: exp(-(i - c)^2 / (2 sd^2)) over their sum, c = (N - 1) / 2, sd = N / 5, as numpy gives them; the
// windows are symmetric, so the first half and the centre
constexpr double kVifG17[9] = {0.007456268901255536, 0.01426550048896806, 0.025031319134073693, 0.040282065814295595, 0.05945262097955645,
                               0.08047510447228295,  0.09990411251845294, 0.11374608465521988,  0.11877384607178972};
constexpr double kVifG9[5] = {0.01897808344053927, 0.055898174540363596, 0.12092090595788882, 0.1921160516399645, 0.2241735688424878};
constexpr double kVifG5[3] = {0.05448868454964294, 0.24420134200323332, 0.4026199468942474};
constexpr double kVifG3[2] = {0.16637851056992245, 0.6672429788601552};
template <int N>
constexpr double vif_g(int i)  // constexpr: the device code and ce_vif_window read it
{
    static_assert(N == 17 || N == 9 || N == 5 || N == 3, "the four windows");
    const int k = i <= N / 2 ? i : N - 1 - i;
    return N == 17 ? kVifG17[k] : N == 9 ? kVifG9[k % 5] : N == 5 ? kVifG5[k % 3] : kVifG3[k % 2];
}

template <int N>
struct vif_geom {
    static constexpr int halo = N - 1;
    static constexpr int in_w = kVifTileW + halo, in_h = kVifTileH + halo;
    static constexpr int in_len = in_w * in_h;          // samples a side in LDS
    static constexpr int col_len = in_w * kVifTileH;    // column-filtered values a stream
    static_assert(in_w % 2 == 0, "rows of the column-filtered streams start 16-byte aligned");
};

// what a sample is staged as: the pyramid's f64, or f32 for a plane's integer sample times 2^(8 - d)
template <class SAMPLE>
using vif_stage_t = typename std::conditional<sizeof(SAMPLE) == 8, double, float>::type;

struct alignas(16) vif_d2 {
    double a, b;
};

// One scale of pairs [first, ...), every plane: blockIdx.y = (pair - first) * n_planes + plane, blockIdx.x the tile
struct vif_args {
    const pf_plane *tab;        // scale 1: [n_refs + n_pairs][3], the references' planes, then the tests'
    const double *pyr;          // scales 2 - 4: plane p of image i at pyr + off[p] + i * w[p] * h[p]
    size_t off[3];
    const uint32_t *pair_ref;   // pair -> reference
    unsigned long long *out;    // [pair][kVifOut]
    uint32_t n_refs, n_planes;
    uint32_t w[3], h[3];        // the planes at this scale; 0 x 0: the plane does not run
    uint32_t maxv, first, scale;  // scale 0 .. 3
    double unit;                // 2^(8 - d)
};

// the block's pair, plane and tile origin; dead where the plane has fewer tiles than the grid's x covers (the grid is sized
// for luma) or does not run
struct vif_where {
    uint32_t pair, plane, x0, y0, vw, vh;  // vw x vh: the plane's positions at this scale
    bool live;
};
template <int N>
__device__ __forceinline__ vif_where vif_block(const vif_args &a)
{
    vif_where o;
    o.pair = a.first + blockIdx.y / a.n_planes, o.plane = blockIdx.y % a.n_planes;
    const uint32_t w = a.w[o.plane], h = a.h[o.plane];
    o.live = w >= (uint32_t)N && h >= (uint32_t)N;
    o.vw = o.live ? w - (N - 1) : 0, o.vh = o.live ? h - (N - 1) : 0;
    const uint32_t tiles_x = (o.vw + kVifTileW - 1) / kVifTileW, tiles_y = (o.vh + kVifTileH - 1) / kVifTileH;
    o.live = o.live && blockIdx.x < tiles_x * tiles_y;
    o.x0 = o.live ? (blockIdx.x % tiles_x) * kVifTileW : 0, o.y0 = o.live ? (blockIdx.x / tiles_x) * kVifTileH : 0;
    return o;
}

// Before the first barrier.  s_in: [2][in_len], the reference's tile, then the test's.
template <int N, class SAMPLE>
__device__ __forceinline__ void vif_stage(const vif_args &a, vif_stage_t<SAMPLE> *s_in)
{
    using G = vif_geom<N>;
    const vif_where o = vif_block<N>(a);
    if (!o.live) return;
    const uint32_t w = a.w[o.plane], h = a.h[o.plane];
    const size_t rs = a.pair_ref[o.pair], ts = (size_t)a.n_refs + o.pair;
    for (int i = threadIdx.x; i < G::in_len; i += kVifThreads) {
        const uint32_t gy = o.y0 + i / G::in_w, gx = o.x0 + i % G::in_w;
        vif_stage_t<SAMPLE> x = 0, y = 0;
        if (gy < h && gx < w) {
            if constexpr (sizeof(SAMPLE) == 8) {
                const size_t plane = (size_t)w * h, at = (size_t)gy * w + gx;
                x = a.pyr[a.off[o.plane] + rs * plane + at], y = a.pyr[a.off[o.plane] + ts * plane + at];
            } else {
                x = (float)((double)pf_sample<SAMPLE>(a.tab[rs * 3 + o.plane], gx, gy, a.maxv) * a.unit);
                y = (float)((double)pf_sample<SAMPLE>(a.tab[ts * 3 + o.plane], gx, gy, a.maxv) * a.unit);
            }
        }
        s_in[i] = x, s_in[G::in_len + i] = y;
    }
}

// Between the barriers: s_col[stream][r][c] = ((g[0] p[r][c] + g[1] p[r + 1][c]) + g[2] p[r + 2][c]) + ... for the five streams,
// U x (T + N - 1) values each.
template <int N, class STAGE>
__device__ __forceinline__ void vif_columns(const vif_args &a, const STAGE *s_in, double *s_col)
{
    using G = vif_geom<N>;
    if (!vif_block<N>(a).live) return;
    for (int j = threadIdx.x; j < G::col_len; j += kVifThreads) {
        double v[kVifStreams];
#pragma unroll
        for (int i = 0; i < N; i++) {
            const double x = (double)s_in[j + i * G::in_w], y = (double)s_in[G::in_len + j + i * G::in_w], g = vif_g<N>(i);
            const double t[kVifStreams] = {g * x, g * y, g * (x * x), g * (y * y), g * (x * y)};
#pragma unroll
            for (int k = 0; k < kVifStreams; k++) v[k] = i == 0 ? t[k] : v[k] + t[k];
        }
#pragma unroll
        for (int k = 0; k < kVifStreams; k++) s_col[k * G::col_len + j] = v[k];
    }
}

// One position from its five filtered values: q[0] = qa, q[1] = qb (include/ce_metrics.h, "Per scale and position", steps
// 1 - 7, and "Logarithm")
__device__ __forceinline__ void vif_position(const double f[kVifStreams], unsigned long long q[2])
{
    const double mu1 = f[0], mu2 = f[1];
    double s1 = f[2] - mu1 * mu1, s2 = f[3] - mu2 * mu2;
    const double s12 = f[4] - mu1 * mu2;
    if (s1 < 0.0) s1 = 0.0;
    if (s2 < 0.0) s2 = 0.0;
    double g = s12 / (s1 + 1e-10);
    double sv = s2 - g * s12;
    if (s1 < 1e-10) g = 0.0, sv = s2, s1 = 0.0;
    if (s2 < 1e-10) g = 0.0, sv = 0.0;
    if (g < 0.0) sv = s2, g = 0.0;
    if (sv <= 1e-10) sv = 1e-10;
    const double va = 1.0 + ((g * g) * s1) / (sv + 2.0), vb = 1.0 + s1 / 2.0;
    q[0] = (unsigned long long)__builtin_rint(ln_fixed(va) * 16777216.0);
    q[1] = (unsigned long long)__builtin_rint(ln_fixed(vb) * 16777216.0);
}

// After the second barrier: the lane's two integers, acc = sum qa, sum qb over those of its four outputs that are positions of
// the plane (0 in a dead block).  N + 1 values of each stream, read as 16-byte pairs.
template <int N>
__device__ __forceinline__ void vif_lane(const vif_args &a, const double *s_col, unsigned long long acc[2])
{
    using G = vif_geom<N>;
    acc[0] = acc[1] = 0;
    const vif_where o = vif_block<N>(a);
    if (!o.live) return;
    const int lx = (threadIdx.x % (kVifTileW / 2)) * 2;
    const uint32_t gx = o.x0 + lx;
    if (gx >= o.vw) return;
    for (int ly = threadIdx.x / (kVifTileW / 2); ly < kVifTileH; ly += kVifTileH / 2) {
        if (o.y0 + ly >= o.vh) break;
        double f0[kVifStreams], f1[kVifStreams];
#pragma unroll
        for (int k = 0; k < kVifStreams; k++) {
            const vif_d2 *row = reinterpret_cast<const vif_d2 *>(s_col + k * G::col_len + ly * G::in_w + lx);
            double v[N + 1];
#pragma unroll
            for (int i = 0; i < (N + 1) / 2; i++) {
                const vif_d2 d = row[i];
                v[2 * i] = d.a, v[2 * i + 1] = d.b;
            }
            double o0 = vif_g<N>(0) * v[0], o1 = vif_g<N>(0) * v[1];
#pragma unroll
            for (int i = 1; i < N; i++) {
                o0 = o0 + vif_g<N>(i) * v[i];
                o1 = o1 + vif_g<N>(i) * v[i + 1];
            }
            f0[k] = o0, f1[k] = o1;
        }
        unsigned long long q[2];
        vif_position(f0, q);
        acc[0] += q[0], acc[1] += q[1];
        if (gx + 1 < o.vw) {
            vif_position(f1, q);
            acc[0] += q[0], acc[1] += q[1];
        }
    }
}

// One scale of images [first, ...), every plane, filtered and decimated into the next: blockIdx.y = (image - first) * n_planes
// + plane
struct vif_reduce_args {
    const pf_plane *tab;    // scale 1 -> 2: as vif_args
    const double *src;      // else: plane p of image i at src + src_off[p] + i * w[p] * h[p]
    double *dst;            // plane p of image i at dst + dst_off[p] + i * ow[p] * oh[p]
    size_t src_off[3], dst_off[3];
    uint32_t n_planes, maxv, first;
    uint32_t w[3], h[3];    // the source planes; 0 x 0: the plane does not run
    uint32_t ow[3], oh[3];  // ow = (w - N + 2) / 2, oh alike
    double unit;
};

// the reduce kernel's tile: R x R outputs a block, one a thread, from (2 R - 2 + N)^2 source samples
constexpr int kVifReduceTile = 16;
static_assert(kVifThreads == kVifReduceTile * kVifReduceTile, "one lane per output");
template <int N>
struct vif_reduce_geom {
    static constexpr int in_w = 2 * kVifReduceTile - 2 + N;  // source samples a row of the tile, and rows
    static constexpr int in_len = in_w * in_w;
    static constexpr int col_len = kVifReduceTile * in_w;     // column-filtered values: the even rows only
};

// the block's image, plane and tile origin (in outputs); dead where the plane has fewer tiles than the grid's x covers (the
// grid is sized for luma) or does not run
struct vif_reduce_where {
    size_t img;
    uint32_t plane, x0, y0;
    bool live;
};
__device__ __forceinline__ vif_reduce_where vif_reduce_block(const vif_reduce_args &a)
{
    vif_reduce_where o;
    o.img = (size_t)a.first + blockIdx.y / a.n_planes, o.plane = blockIdx.y % a.n_planes;
    const uint32_t tiles_x = (a.ow[o.plane] + kVifReduceTile - 1) / kVifReduceTile, tiles_y = (a.oh[o.plane] + kVifReduceTile - 1) / kVifReduceTile;
    o.live = blockIdx.x < tiles_x * tiles_y;
    o.x0 = o.live ? (blockIdx.x % tiles_x) * kVifReduceTile : 0, o.y0 = o.live ? (blockIdx.x / tiles_x) * kVifReduceTile : 0;
    return o;
}

// Before the first barrier: the source samples of the tile, zeros outside the plane (those feed masked outputs only)
template <int N, class SAMPLE>
__device__ __forceinline__ void vif_reduce_stage(const vif_reduce_args &a, vif_stage_t<SAMPLE> *s_in)
{
    using G = vif_reduce_geom<N>;
    const vif_reduce_where o = vif_reduce_block(a);
    if (!o.live) return;
    const uint32_t w = a.w[o.plane], h = a.h[o.plane];
    for (int i = threadIdx.x; i < G::in_len; i += kVifThreads) {
        const uint32_t gy = 2 * o.y0 + i / G::in_w, gx = 2 * o.x0 + i % G::in_w;
        vif_stage_t<SAMPLE> v = 0;
        if (gy < h && gx < w) {
            if constexpr (sizeof(SAMPLE) == 8) v = a.src[a.src_off[o.plane] + (o.img * h + gy) * w + gx];
            else v = (float)((double)pf_sample<SAMPLE>(a.tab[o.img * 3 + o.plane], gx, gy, a.maxv) * a.unit);
        }
        s_in[i] = v;
    }
}

// Between the barriers: the filter down the columns at the even rows, s_col[Y][c] = ((g[0] p[2Y][c] + g[1] p[2Y + 1][c]) + ...
template <int N, class STAGE>
__device__ __forceinline__ void vif_reduce_columns(const vif_reduce_args &a, const STAGE *s_in, double *s_col)
{
    using G = vif_reduce_geom<N>;
    if (!vif_reduce_block(a).live) return;
    for (int j = threadIdx.x; j < G::col_len; j += kVifThreads) {
        const int Y = j / G::in_w, c = j % G::in_w;
        double v = vif_g<N>(0) * (double)s_in[2 * Y * G::in_w + c];
#pragma unroll
        for (int i = 1; i < N; i++) v = v + vif_g<N>(i) * (double)s_in[(2 * Y + i) * G::in_w + c];
        s_col[j] = v;
    }
}

// After the second barrier: the lane's output, the filter along the row at the even columns
template <int N>
__device__ __forceinline__ void vif_reduce_rows(const vif_reduce_args &a, const double *s_col)
{
    using G = vif_reduce_geom<N>;
    const vif_reduce_where o = vif_reduce_block(a);
    if (!o.live) return;
    const uint32_t lx = threadIdx.x % kVifReduceTile, ly = threadIdx.x / kVifReduceTile;
    const uint32_t X = o.x0 + lx, Y = o.y0 + ly, ow = a.ow[o.plane], oh = a.oh[o.plane];
    if (X >= ow || Y >= oh) return;
    const double *row = s_col + ly * G::in_w + 2 * lx;
    double v = vif_g<N>(0) * row[0];
#pragma unroll
    for (int j = 1; j < N; j++) v = v + vif_g<N>(j) * row[j];
    a.dst[a.dst_off[o.plane] + (o.img * oh + Y) * ow + X] = v;
}

}  // namespace
