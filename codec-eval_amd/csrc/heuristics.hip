// Image heuristics on gfx950 — replaces compute_heuristics (crates/codec-compare/src/image_heuristics.rs:76-305) and the
// statistics of analyze (crates/codec-compare/src/analyze_image.rs:48-118).
//
// Every per-pixel and per-block value is the reference's f32 arithmetic (the file is built with -ffp-contract=off and
// correctly rounded f32 division and square root), so every threshold decision, count and maximum equals the
// reference's.  The whole-image sums add the same f32 terms in f64, in an order fixed by the image's shape alone (a
// tile's pixels in a fixed lane order, tiles in a fixed tree), and are rounded once to f32 (ce_metrics.h).
//
// Four launches, each covering every image of the call:
//   k_heur_tiles<false>   one workgroup per 64 x 64 tile: gray with a 1-pixel halo in LDS; per tile f64 sums, u32 counts
//                         and the edge maximum; each 8 x 8 block (tiles are multiples of 8, so no block straddles two)
//                         is walked sequentially by one lane
//   k_heur_reduce<false>  one workgroup per image: the tiles in fixed order -> the means and the exact fields
//   k_heur_tiles<true>    the (v - mean)^2 terms of the variances (the RGB8 image is read again; block variances are
//                         recomputed by the same sequential walk, bit-identical to the first pass, instead of kept)
//   k_heur_reduce<true>   the variances and standard deviations
#include <cstring>

#include "ce_internal.h"

namespace {

constexpr int kTileW = 64, kTileH = 64, kThreads = 256;
constexpr int kLdsW = kTileW + 2, kLdsH = kTileH + 2;
constexpr int kBlocksX = kTileW / 8, kBlocksY = kTileH / 8;
static_assert(kTileW % 8 == 0 && kTileH % 8 == 0, "8x8 blocks must not straddle tiles");
static_assert(kBlocksX * kBlocksY <= kThreads, "one lane per block");

// slots of a tile's partials (f64; counts are exact integers there).  Pass 1: sums, counts, the maximum
enum {
    S_GRAY, S_R, S_G, S_B, S_SAT, S_EDGE, S_CONTRAST, S_HCX, S_VCX, S_DCX, S_BVAR,
    C_EDGE30, C_LOWF, C_HIGHF, C_FLAT, C_LOWVAR, C_MIDVAR, C_HIGHVAR, C_DETAIL, C_OVER1000,
    M_EDGE,
    kSlots
};
constexpr int kSums1 = C_EDGE30, kCounts1 = M_EDGE - C_EDGE30;
// pass 2: the (v - mean)^2 sums; the means pass 1 leaves per image, in the same order
enum { D_GRAY, D_R, D_G, D_B, D_SAT, D_CONTRAST, D_BVAR, kSlots3 };
constexpr int kMeans = 8;

__device__ __forceinline__ float gray_of(uint32_t r, uint32_t g, uint32_t b)
{
    return 0.299f * (float)r + 0.587f * (float)g + 0.114f * (float)b;  // image_heuristics.rs:87, left to right
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// count as f32 the way `n as f32` rounds a usize (exact through f64 below 2^53)
__device__ __forceinline__ float f32_of(double n) { return (float)n; }

// one 8 x 8 block's variance from the LDS tile, as image_heuristics.rs:114-131: sequential f32 sums in row-major order
__device__ __forceinline__ float block_variance(const float (*g)[kLdsW], int ly0, int lx0)
{
    float s = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 8; dy++)
#pragma unroll
        for (int dx = 0; dx < 8; dx++) s += g[ly0 + dy][lx0 + dx];
    const float mean = s / 64.0f;
    float q = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 8; dy++)
#pragma unroll
        for (int dx = 0; dx < 8; dx++) {
            const float d = g[ly0 + dy][lx0 + dx] - mean;
            q += d * d;
        }
    return q / 64.0f;
}

template <bool DEV>
__global__ __launch_bounds__(kThreads) void k_heur_tiles(const uint8_t *__restrict__ imgs, size_t img_stride, uint32_t w,
                                                         uint32_t h, uint32_t tiles_x, uint32_t n_tiles,
                                                         const float *__restrict__ means, double *__restrict__ part)
{
    __shared__ float g[kLdsH][kLdsW];
    __shared__ double red[kThreads / 64][kSlots];
    const uint32_t img = blockIdx.x / n_tiles, tile = blockIdx.x - img * n_tiles;
    const int x0 = (int)((tile % tiles_x) * kTileW), y0 = (int)((tile / tiles_x) * kTileH);
    const uint8_t *src = imgs + (size_t)img * img_stride;
    const int tid = threadIdx.x;
    float m[kMeans] = {};
    if (DEV)
#pragma unroll
        for (int k = 0; k < kMeans; k++) m[k] = means[(size_t)img * kMeans + k];

    double s[kSums1] = {};
    uint32_t c[kCounts1] = {};
    float emax = 0.0f;  // fold(0.0, max), image_heuristics.rs:107

    // stage gray (tile + halo; 0 outside the image, never read there) and take the per-pixel terms of the tile's own pixels
    for (int i = tid; i < kLdsH * kLdsW; i += kThreads) {
        const int ly = i / kLdsW, lx = i - ly * kLdsW;
        const int x = x0 + lx - 1, y = y0 + ly - 1;
        float v = 0.0f;
        if (x >= 0 && x < (int)w && y >= 0 && y < (int)h) {
            const uint8_t *p = src + ((size_t)y * w + x) * 3;
            const uint32_t r = p[0], gg = p[1], b = p[2];
            v = gray_of(r, gg, b);
            if (lx >= 1 && lx <= kTileW && ly >= 1 && ly <= kTileH) {
                // saturation, image_heuristics.rs:187-195
                const float mx = (float)max(max(r, gg), b), mn = (float)min(min(r, gg), b);
                const float sat = mx > 0.0f ? (mx - mn) / mx : 0.0f;
                if (!DEV) {
                    s[S_GRAY] += (double)v;
                    s[S_R] += (double)r;
                    s[S_G] += (double)gg;
                    s[S_B] += (double)b;
                    s[S_SAT] += (double)sat;
                } else {
                    const float d0 = v - m[D_GRAY], d1 = (float)r - m[D_R], d2 = (float)gg - m[D_G], d3 = (float)b - m[D_B],
                                d4 = sat - m[D_SAT];
                    const float q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3, q4 = d4 * d4;
                    s[D_GRAY] += (double)q0;
                    s[D_R] += (double)q1;
                    s[D_G] += (double)q2;
                    s[D_B] += (double)q3;
                    s[D_SAT] += (double)q4;
                }
            }
        }
        g[ly][lx] = v;
    }
    __syncthreads();

    for (int i = tid; i < kTileW * kTileH; i += kThreads) {
        const int ly = i / kTileW + 1, lx = i % kTileW + 1;
        const int x = x0 + lx - 1, y = y0 + ly - 1;
        if (x >= (int)w || y >= (int)h) continue;
        const float v = g[ly][lx];
        if (!DEV && x + 1 < (int)w) {  // adjacent differences over every row, image_heuristics.rs:203-216
            const float diff = fabsf(g[ly][lx + 1] - v);
            if (diff < 10.0f) c[C_LOWF - C_EDGE30]++;
            else if (diff > 30.0f) c[C_HIGHF - C_EDGE30]++;
        }
        if (x < 1 || x + 1 >= (int)w || y < 1 || y + 1 >= (int)h) continue;
        // 3x3 contrast, image_heuristics.rs:228-243
        float lo = v, hi = v;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                lo = fminf(lo, g[ly + dy][lx + dx]);
                hi = fmaxf(hi, g[ly + dy][lx + dx]);
            }
        const float contrast = hi - lo;
        if (!DEV) {
            // gradients and edge strength (image_heuristics.rs:96-104), directional complexity (:262-271)
            const float gx = g[ly][lx + 1] - g[ly][lx - 1];
            const float gy = g[ly + 1][lx] - g[ly - 1][lx];
            const float strength = sqrtf(gx * gx + gy * gy);
            s[S_EDGE] += (double)strength;
            emax = fmaxf(emax, strength);
            if (strength > 30.0f) c[C_EDGE30 - C_EDGE30]++;
            s[S_CONTRAST] += (double)contrast;
            s[S_HCX] += (double)fabsf(gx);
            s[S_VCX] += (double)fabsf(gy);
            s[S_DCX] += (double)fabsf(g[ly + 1][lx + 1] - g[ly - 1][lx - 1]);
        } else {
            const float d = contrast - m[D_CONTRAST], q = d * d;
            s[D_CONTRAST] += (double)q;
        }
    }

    if (tid < kBlocksX * kBlocksY) {
        const int bx = tid % kBlocksX, by = tid / kBlocksX;
        const uint32_t gbx = (uint32_t)x0 / 8 + bx, gby = (uint32_t)y0 / 8 + by;
        if (gbx < w / 8 && gby < h / 8) {  // whole blocks only, image_heuristics.rs:111-112
            const float var = block_variance(g, 1 + by * 8, 1 + bx * 8);
            if (!DEV) {
                s[S_BVAR] += (double)var;
                // thresholds of image_heuristics.rs:142-160 (flat and low overlap) and analyze_image.rs:94
                c[C_FLAT - C_EDGE30] += var < 100.0f;
                c[C_LOWVAR - C_EDGE30] += var < 500.0f;
                c[C_MIDVAR - C_EDGE30] += var >= 500.0f && var < 2000.0f;
                c[C_HIGHVAR - C_EDGE30] += var >= 2000.0f && var < 5000.0f;
                c[C_DETAIL - C_EDGE30] += var >= 5000.0f;
                c[C_OVER1000 - C_EDGE30] += var > 1000.0f;
            } else {
                const float d = var - m[D_BVAR], q = d * d;
                s[D_BVAR] += (double)q;
            }
        }
    }

    // fixed-order reduction: butterfly within each wave, then the four waves in order
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int n_sums = DEV ? (int)kSlots3 : kSums1;
#pragma unroll
    for (int k = 0; k < n_sums; k++) {
        const double t = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = t;
    }
    if (!DEV) {
#pragma unroll
        for (int k = 0; k < kCounts1; k++) {
            const uint32_t t = wave_sum(c[k]);
            if (lane == 0) red[wave][C_EDGE30 + k] = (double)t;
        }
        const float t = wave_max(emax);
        if (lane == 0) red[wave][M_EDGE] = (double)t;
    }
    __syncthreads();
    const int n_out = DEV ? (int)kSlots3 : (int)kSlots;
    if (tid < n_out) {
        double t = red[0][tid];
        for (int k = 1; k < kThreads / 64; k++) t = (!DEV && tid == M_EDGE) ? fmax(t, red[k][tid]) : t + red[k][tid];
        part[(size_t)blockIdx.x * kSlots + tid] = t;
    }
}

template <bool DEV>
__global__ __launch_bounds__(kThreads) void k_heur_reduce(const double *__restrict__ part, uint32_t n_tiles, uint32_t w,
                                                          uint32_t h, float *__restrict__ means,
                                                          ce_image_heuristics *__restrict__ out)
{
    __shared__ double red[kThreads / 64][kSlots];
    const uint32_t img = blockIdx.x;
    const double *p = part + (size_t)img * n_tiles * kSlots;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int n_slots = DEV ? (int)kSlots3 : (int)kSlots;
    for (int k = 0; k < n_slots; k++) {
        const bool is_max = !DEV && k == M_EDGE;
        double a = 0.0;
        for (uint32_t t = tid; t < n_tiles; t += kThreads) a = is_max ? fmax(a, p[(size_t)t * kSlots + k]) : a + p[(size_t)t * kSlots + k];
        if (is_max)
            for (int off = 32; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off, 64));
        else
            a = wave_sum(a);
        if (lane == 0) red[wave][k] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[kSlots];
    for (int k = 0; k < n_slots; k++) {
        double t = red[0][k];
        for (int q = 1; q < kThreads / 64; q++) t = (!DEV && k == M_EDGE) ? fmax(t, red[q][k]) : t + red[q][k];
        tot[k] = t;
    }
    // the reference's divisors, image_heuristics.rs:89-275
    const uint64_t n_px = (uint64_t)w * h, n_in = (uint64_t)(w - 2) * (h - 2), n_blk = (uint64_t)(w / 8) * (h / 8);
    const float pixels = f32_of((double)n_px);
    const float inner = f32_of((double)(n_in > 0 ? n_in : 1));  // edge_strengths.len().max(1), local_contrasts.len().max(1)
    const float n_cx = f32_of((double)n_in);                     // ((width - 2) * (height - 2)) as f32
    const float blocks = f32_of((double)(n_blk > 0 ? n_blk : 1));  // block_variances.len().max(1)
    ce_image_heuristics &o = out[img];
    float *mu = means + (size_t)img * kMeans;
    if (!DEV) {
        o.width = w;
        o.height = h;
        o.pixels = n_px;
        o.mean_luminance = f32_of(tot[S_GRAY]) / pixels;
        o.edge_strength_mean = f32_of(tot[S_EDGE]) / inner;
        o.edge_strength_max = (float)tot[M_EDGE];
        o.edge_density = f32_of(tot[C_EDGE30]) / inner;
        o.flat_block_pct = 100.0f * f32_of(tot[C_FLAT]) / blocks;
        o.low_var_block_pct = 100.0f * f32_of(tot[C_LOWVAR]) / blocks;
        o.mid_var_block_pct = 100.0f * f32_of(tot[C_MIDVAR]) / blocks;
        o.high_var_block_pct = 100.0f * f32_of(tot[C_HIGHVAR]) / blocks;
        o.detail_block_pct = 100.0f * f32_of(tot[C_DETAIL]) / blocks;
        o.analyze_detail_block_pct = 100.0f * f32_of(tot[C_OVER1000]) / blocks;
        o.block_variance_mean = f32_of(tot[S_BVAR]) / blocks;
        o.saturation_mean = f32_of(tot[S_SAT]) / pixels;
        // the reference counts transitions in f32 accumulators (+= 1.0): they stop at 2^24 (image_heuristics.rs:200-210)
        const float low = f32_of(fmin(tot[C_LOWF], 16777216.0)), high = f32_of(fmin(tot[C_HIGHF], 16777216.0));
        const float transitions = f32_of((double)((uint64_t)(w - 1) * h));
        o.low_freq_energy = low / transitions;
        o.high_freq_energy = high / transitions;
        o.freq_ratio = o.low_freq_energy > 0.0f ? o.high_freq_energy / o.low_freq_energy : o.high_freq_energy;
        o.local_contrast_mean = f32_of(tot[S_CONTRAST]) / inner;
        o.horizontal_complexity = f32_of(tot[S_HCX]) / n_cx;
        o.vertical_complexity = f32_of(tot[S_VCX]) / n_cx;
        o.diagonal_complexity = f32_of(tot[S_DCX]) / n_cx;
        mu[D_GRAY] = o.mean_luminance;
        mu[D_R] = f32_of(tot[S_R]) / pixels;
        mu[D_G] = f32_of(tot[S_G]) / pixels;
        mu[D_B] = f32_of(tot[S_B]) / pixels;
        mu[D_SAT] = o.saturation_mean;
        mu[D_CONTRAST] = o.local_contrast_mean;
        mu[D_BVAR] = o.block_variance_mean;
        mu[kSlots3] = 0.0f;
    } else {
        o.luminance_variance = f32_of(tot[D_GRAY]) / pixels;
        o.luminance_std = sqrtf(o.luminance_variance);
        o.block_variance_std = sqrtf(f32_of(tot[D_BVAR]) / blocks);
        const float r_var = f32_of(tot[D_R]) / pixels, g_var = f32_of(tot[D_G]) / pixels, b_var = f32_of(tot[D_B]) / pixels;
        o.color_variance = (r_var + g_var + b_var) / 3.0f;
        o.saturation_std = sqrtf(f32_of(tot[D_SAT]) / pixels);
        o.local_contrast_std = sqrtf(f32_of(tot[D_CONTRAST]) / inner);
    }
}

}  // namespace

int ce_image_heuristics_run(ce_ctx *ctx, const uint8_t *d_imgs, size_t img_stride, uint32_t w, uint32_t h, uint32_t n,
                            ce_image_heuristics *out)
{
    const uint32_t tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y;
    if (n_tiles * n > 0x7fffffffull) {
        ctx->err = "image heuristics: too many tiles for one launch";
        return CE_ERR_INVALID_ARG;
    }
    // scratch: [n][tiles][kSlots] f64 partials | [n][kMeans] f32 means | [n] results
    const size_t part_bytes = (size_t)n * n_tiles * kSlots * sizeof(double);
    const size_t mean_bytes = (size_t)n * kMeans * sizeof(float);
    const size_t out_bytes = (size_t)n * sizeof(ce_image_heuristics);
    const size_t need = part_bytes + mean_bytes + out_bytes;
    if (ctx->heur_d_cap < need) {
        CE_HIP(ctx, hipFree(ctx->heur_d));  // every earlier call synchronised before it returned
        ctx->heur_d = nullptr;
        ctx->heur_d_cap = 0;
        CE_HIP(ctx, hipMalloc((void **)&ctx->heur_d, need));
        ctx->heur_d_cap = need;
    }
    if (ctx->heur_h_cap < out_bytes) {
        if (ctx->heur_h) CE_HIP(ctx, hipHostFree(ctx->heur_h));
        ctx->heur_h = nullptr;
        ctx->heur_h_cap = 0;
        CE_HIP(ctx, hipHostMalloc((void **)&ctx->heur_h, out_bytes, hipHostMallocDefault));
        ctx->heur_h_cap = out_bytes;
    }
    double *part = reinterpret_cast<double *>(ctx->heur_d);
    float *means = reinterpret_cast<float *>(ctx->heur_d + part_bytes);
    ce_image_heuristics *d_out = reinterpret_cast<ce_image_heuristics *>(ctx->heur_d + part_bytes + mean_bytes);
    const hipStream_t st = ctx->stream;
    const dim3 tiles_grid((uint32_t)(n_tiles * n));
    CE_LAUNCH_ON(ctx, st, "heur_tiles", k_heur_tiles<false>, tiles_grid, dim3(kThreads), 0, d_imgs, img_stride, w, h, tiles_x,
                 (uint32_t)n_tiles, means, part);
    CE_LAUNCH_ON(ctx, st, "heur_reduce", k_heur_reduce<false>, dim3(n), dim3(kThreads), 0, part, (uint32_t)n_tiles, w, h, means,
                 d_out);
    CE_LAUNCH_ON(ctx, st, "heur_tiles_dev", k_heur_tiles<true>, tiles_grid, dim3(kThreads), 0, d_imgs, img_stride, w, h, tiles_x,
                 (uint32_t)n_tiles, means, part);
    CE_LAUNCH_ON(ctx, st, "heur_reduce_dev", k_heur_reduce<true>, dim3(n), dim3(kThreads), 0, part, (uint32_t)n_tiles, w, h,
                 means, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->heur_h, d_out, out_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // also drains what was queued when a step above failed
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        ctx->err = std::string("image heuristics: ") + hipGetErrorString(e);
        return CE_ERR_BACKEND;
    }
    std::memcpy(out, ctx->heur_h, out_bytes);
    return CE_OK;
}
