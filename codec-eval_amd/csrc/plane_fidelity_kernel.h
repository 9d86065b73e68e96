// The device code of the plane-domain scores (plane_fidelity.hip; include/ce_metrics.h: ce_yuv_plane_fidelity; DESIGN.md
// section 28), kept like msssim_kernel.h free of anything but the HIP keywords and blockIdx / threadIdx / gridDim, so that
// tests/cpp/plane_fidelity_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.  A
// decoder's Y, Cb and Cr planes are scored where they lie: a plane of an image is a pf_plane - base, pitch, the step from a
// sample to its right neighbour (2 in the interleaved CbCr plane of NV12 / P010, where Cr's base is one sample past Cb's) and
// the shift of MSB-aligned samples - and a sample is min(v >> shift, 2^d - 1), as the ingest reads it.
//   pf_sse_thread   a thread's share of sum (x - y)^2 over one plane of one pair (a launch covers the planes of its pairs): a wave walks rows, 16 bytes of samples a lane
//                   where both rows admit it, sample by sample where they do not - chosen per row from the addresses
//   pf_stage        msssim_kernel.h's 42 x 26 tiles filled from a pitched plane (level 0) or from the f32 pyramid; mss_columns,
//                   mss_lane and mss_quantise then run unchanged (they take only the tile origin, the level's size and C1, C2
//                   from mss_args)
//   pf_pool_sample  one sample of the next level, section 27's padded 2 x 2 mean
// The reductions across lanes stay in plane_fidelity.hip.
#pragma once

#include "msssim_kernel.h"

namespace {

constexpr uint32_t kPfThreads = 256, kPfWaves = kPfThreads / 64;
constexpr uint32_t kPfOut = 3 + 3 * 5 * 2;  // u64 a pair: sse[3], then [plane][level][2] = ssim_q, cs_q

// one plane of one image
struct pf_plane {
    const uint8_t *base;  // the first sample
    size_t pitch;         // bytes from a row to the next
    uint32_t step;        // samples from a sample to its right neighbour: 1, or 2 in an interleaved CbCr plane
    uint32_t shift;       // 16 - d for MSB-aligned u16 samples, else 0
};

template <int BPS>
struct pf_sample_of {
    using type = uint8_t;
};
template <>
struct pf_sample_of<2> {
    using type = uint16_t;
};

template <class SAMPLE>
__device__ __forceinline__ uint32_t pf_sample(const pf_plane &pl, uint32_t x, uint32_t y, uint32_t maxv)
{
    const uint32_t v = *reinterpret_cast<const SAMPLE *>(pl.base + (size_t)y * pl.pitch + (size_t)x * pl.step * sizeof(SAMPLE)) >> pl.shift;
    return v < maxv ? v : maxv;
}

// ---- the squared error of one plane ------------------------------------------------------------------------------------------

struct pf_sse_args {
    const pf_plane *tab;        // [n_refs + n_pairs][3]: the references' planes, then the tests'
    const uint32_t *pair_ref;   // pair -> reference
    unsigned long long *out;    // [pair][kPfOut]
    uint32_t n_refs, n_planes;  // blockIdx.y = (pair - first) * n_planes + plane, plane 0, 1, 2 = Y, Cb, Cr
    uint32_t w[3], h[3];        // the planes' sizes
    uint32_t maxv, first;       // 2^d - 1
};

// the block's pair and plane
struct pf_where {
    uint32_t pair, plane;
};
__device__ __forceinline__ pf_where pf_sse_block(const pf_sse_args &a)
{
    pf_where o;
    o.pair = a.first + blockIdx.y / a.n_planes, o.plane = blockIdx.y % a.n_planes;
    return o;
}

// May the wide path read this row?  A planar row must start on 16 bytes.  An interleaved row is read as whole 32-byte pieces of
// CbCr pairs from Cb's first sample, so Cb's rows must start on 16 bytes and Cr's one sample past that.
template <int BPS>
__device__ __forceinline__ bool pf_wide_ok(const uint8_t *row, uint32_t step, uint32_t plane)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(row) & 15u;
    return at == (step == 2 && plane == 2 ? (uintptr_t)BPS : 0u);
}

// samples [i * 16 / BPS, (i + 1) * 16 / BPS) of a row that pf_wide_ok admits, as they lie in memory: 16 bytes of a planar row,
// or every other sample of 32 bytes of an interleaved one (all of them inside the row: the row holds 2 * w samples)
template <int BPS>
__device__ __forceinline__ uint4 pf_load16(const uint8_t *row, uint32_t step, size_t i)
{
    if (step == 1) return reinterpret_cast<const uint4 *>(row)[i];
    const uintptr_t at = reinterpret_cast<uintptr_t>(row) & 15u;  // 0: Cb, BPS: Cr
    const uint4 *q = reinterpret_cast<const uint4 *>(row - at) + 2 * i;
    const uint4 lo = q[0], hi = q[1];
    const uint32_t s = 8u * (uint32_t)at;
    uint4 o;
    if (BPS == 1) {
        auto pick = [s](uint32_t d0, uint32_t d1) {
            d0 >>= s, d1 >>= s;
            return (d0 & 0xffu) | ((d0 >> 8) & 0xff00u) | ((d1 & 0xffu) << 16) | ((d1 << 8) & 0xff000000u);
        };
        o.x = pick(lo.x, lo.y), o.y = pick(lo.z, lo.w), o.z = pick(hi.x, hi.y), o.w = pick(hi.z, hi.w);
    } else {
        auto pick = [s](uint32_t d0, uint32_t d1) { return ((d0 >> s) & 0xffffu) | ((d1 >> s) << 16); };
        o.x = pick(lo.x, lo.y), o.y = pick(lo.z, lo.w), o.z = pick(hi.x, hi.y), o.w = pick(hi.z, hi.w);
    }
    return o;
}

// c + the dot product of the four bytes of a and b
__device__ __forceinline__ uint32_t pf_dot4(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int k = 0; k < 32; k += 8) c += ((a >> k) & 0xffu) * ((b >> k) & 0xffu);
    return c;
#endif
}

// sum (x - y)^2 over 16 bytes of samples of either side.  u8 has neither shift nor clamp (msb_aligned is refused at depth 8 and
// 2^8 - 1 is the type's range): sum x^2 + sum y^2 - 2 sum xy in three dot products a dword, as k_psnr_sse; at most 16 * 255^2.
// u16: eight samples through min(v >> shift, maxv); a difference is under 2^12, the eight squares under 2^27.
template <int BPS>
__device__ __forceinline__ uint32_t pf_sse16(const uint4 a, const uint4 b, uint32_t shift_a, uint32_t shift_b, uint32_t maxv)
{
    const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
    if (BPS == 1) {
        uint32_t saa = 0, sbb = 0, sab = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            saa = pf_dot4(wa[k], wa[k], saa);
            sbb = pf_dot4(wb[k], wb[k], sbb);
            sab = pf_dot4(wa[k], wb[k], sab);
        }
        return (saa + sbb) - 2u * sab;
    }
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int half = 0; half < 2; half++) {
            uint32_t x = ((wa[k] >> (16 * half)) & 0xffffu) >> shift_a, y = ((wb[k] >> (16 * half)) & 0xffffu) >> shift_b;
            x = x < maxv ? x : maxv, y = y < maxv ? y : maxv;
            const uint32_t d = x > y ? x - y : y - x;
            sum += d * d;
        }
    }
    return sum;
}

// The thread's share of the block's plane of its pair.  Wave k of the grid's blockIdx.x-th block takes rows 4 blockIdx.x + k,
// + 4 gridDim.x, ... (the grid is sized for luma: on a subsampled plane the later blocks find no row): rows are pitched, and the
// two sides may differ in pitch and step, so rows are walked, not a range of bytes.  Integers: neither the grid nor the order
// matters.
template <int BPS>
__device__ __forceinline__ unsigned long long pf_sse_thread(const pf_sse_args &a)
{
    using SAMPLE = typename pf_sample_of<BPS>::type;
    constexpr uint32_t N = 16 / BPS;  // samples in 16 bytes
    const pf_where o = pf_sse_block(a);
    const uint32_t w = a.w[o.plane], h = a.h[o.plane];
    const pf_plane x = a.tab[(size_t)a.pair_ref[o.pair] * 3 + o.plane], y = a.tab[((size_t)a.n_refs + o.pair) * 3 + o.plane];
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    unsigned long long sse = 0;
    for (uint32_t r = blockIdx.x * kPfWaves + wave; r < h; r += gridDim.x * kPfWaves) {
        const uint8_t *rx = x.base + (size_t)r * x.pitch, *ry = y.base + (size_t)r * y.pitch;
        uint32_t done = 0;
        if (pf_wide_ok<BPS>(rx, x.step, o.plane) && pf_wide_ok<BPS>(ry, y.step, o.plane)) {
            const uint32_t n16 = w / N;
            for (uint32_t i = lane; i < n16; i += 64u)
                sse += pf_sse16<BPS>(pf_load16<BPS>(rx, x.step, i), pf_load16<BPS>(ry, y.step, i), x.shift, y.shift, a.maxv);
            done = n16 * N;
        }
        for (uint32_t c = done + lane; c < w; c += 64u) {
            const uint32_t u = pf_sample<SAMPLE>(x, c, r, a.maxv), v = pf_sample<SAMPLE>(y, c, r, a.maxv);
            const uint32_t d = u > v ? u - v : v - u;
            sse += d * d;
        }
    }
    return sse;
}

// ---- SSIM / MS-SSIM of one plane and level -------------------------------------------------------------------------------------

struct pf_level_args {
    mss_args m;             // w, h, tiles_x, level, c1, c2 of this plane and level, pair_ref, first (blockIdx.y = 0 is pair `first`)
    const pf_plane *tab;    // level 0: as pf_sse_args
    const float *pyr;       // levels 1 - 4: [n_refs + n_pairs][h][w] of this plane and level
    unsigned long long *out;
    uint32_t n_refs, plane, maxv;
};

// Before the first barrier, in mss_stage's place: the tile of the two planes with its halo, zeros outside the plane.  SAMPLE is
// uint8_t / uint16_t for a pitched plane found through the table, float for the pyramid.
template <class SAMPLE>
__device__ __forceinline__ void pf_stage(const pf_level_args &a, float *s_in)
{
    const uint32_t pair = a.m.first + blockIdx.y;
    const uint32_t x0 = (blockIdx.x % a.m.tiles_x) * kMssTileW, y0 = (blockIdx.x / a.m.tiles_x) * kMssTileH;  // mss_block's
    const size_t rs = a.m.pair_ref[pair], ts = (size_t)a.n_refs + pair;
    for (int i = threadIdx.x; i < kMssInLen; i += kMssThreads) {
        const uint32_t gy = y0 + i / kMssInW, gx = x0 + i % kMssInW;
        float x = 0.0f, y = 0.0f;
        if (gy < a.m.h && gx < a.m.w) {
            if constexpr (sizeof(SAMPLE) == 4) {
                const size_t plane = (size_t)a.m.w * a.m.h, at = (size_t)gy * a.m.w + gx;
                x = a.pyr[rs * plane + at], y = a.pyr[ts * plane + at];
            } else {
                x = (float)pf_sample<SAMPLE>(a.tab[rs * 3 + a.plane], gx, gy, a.maxv);
                y = (float)pf_sample<SAMPLE>(a.tab[ts * 3 + a.plane], gx, gy, a.maxv);
            }
        }
        s_in[i] = x, s_in[kMssInLen + i] = y;
    }
}

// One level of one plane of images [first, ...) of the call pooled into the next
struct pf_pool_args {
    const pf_plane *tab;  // level 0 -> 1
    const float *src;     // else: [n_refs + n_pairs][h][w]
    float *dst;           // [n_refs + n_pairs][oh][ow]
    uint32_t plane, maxv;
    uint32_t w, h, ow, oh;  // ow = (w + (w & 1)) / 2, oh alike
    uint32_t first;         // blockIdx.y = 0 is image `first`
};

// dst sample i of image first + blockIdx.y: mss_pool_sample's mean on one plane
template <class SAMPLE>
__device__ __forceinline__ void pf_pool_sample(const pf_pool_args &a, size_t i)
{
    const size_t img = (size_t)a.first + blockIdx.y;
    const uint32_t Y = (uint32_t)(i / a.ow), X = (uint32_t)(i % a.ow);
    const uint32_t pw = a.w & 1u, ph = a.h & 1u;
    double q[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const uint32_t qy = 2 * Y + dy, qx = 2 * X + dx;  // in the padded plane
            double v = 0.0;
            if (qy >= ph && qx >= pw) {
                if constexpr (sizeof(SAMPLE) == 4) v = (double)a.src[(img * a.h + (qy - ph)) * a.w + (qx - pw)];
                else v = (double)pf_sample<SAMPLE>(a.tab[img * 3 + a.plane], qx - pw, qy - ph, a.maxv);
            }
            q[dy][dx] = v;
        }
    a.dst[img * a.ow * a.oh + i] = (float)(((q[0][0] + q[0][1]) + (q[1][0] + q[1][1])) * 0.25);
}

}  // namespace
