// The device code of linear-light compositing (include/ce_metrics.h: ce_batch_set_*_cicp_over and its kin; DESIGN.md section
// 24): an image with alpha is turned into linear light pixel by pixel, as the plain ingest of its kind does, and blended
// there over n_bg solid colours into n_bg consecutive slots of a linear batch.  Kept free of anything but the HIP keywords,
// uint2 / uint4 / float4 and blockIdx / threadIdx, like cicp_kernel.h, whose loads, store and block size it uses, so that
// tests/cpp/over_linear_kernel_host.cpp compiles the same text for the host.  Two frames: k_tagged_over beside k_tagged, with
// the same pixels as its parameter (cicp_px, hlg_px, icc_px, icc_lut_px), and k_linear_over for CE_PIXEL_RGBA_F32.  Every
// product and sum is a separately rounded f32 operation (-ffp-contract=off).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

#include "cicp_kernel.h"

namespace {

// what a frame blends with, beside its pixel's own arguments
struct over_args {
    const float *atab;    // k_tagged_over: atab[k] = float32(k) / float32(maxv), maxv + 1 entries; k_linear_over: unused
    uint32_t n_bg;        // 1 .. CE_MAX_BACKGROUNDS
    size_t slot_floats;   // from one slot to the next: n_pixels * 3
    float bg[CE_MAX_BACKGROUNDS][3];  // linear light, sRGB primaries, finite and within +-CE_LINEAR_MAX
};

// steps 3 and 4 of the definition on one sample: v the pixel's linear value, t its coverage and u = 1 - t
__device__ __forceinline__ float over_blend(float v, float bg, float t, float u)
{
    const float p = v * t, q = bg * u;
    const float o = t == 1.0f ? v : (t == 0.0f ? bg : p + q);
    return linear_clamp(o);
}

// the premultiplied form: v already holds colour * coverage
__device__ __forceinline__ float over_blend_premul(float v, float bg, float u)
{
    const float q = bg * u;
    const float o = u == 0.0f ? v : v + q;
    return linear_clamp(o);
}

// a float image's coverage: NaN -> 0, then [0, 1]
__device__ __forceinline__ float over_coverage(float a)
{
    if (a != a) return 0.0f;
    return a > 1.0f ? 1.0f : (a < 0.0f ? 0.0f : a);
}

// the alpha sample of pixel p of an RGBA8 / RGBA16 image (the tail; cicp_load_pixel reads the three colours)
template <int FMT>
__device__ __forceinline__ uint32_t over_load_alpha(const void *src, size_t p)
{
    return FMT == CE_PIXEL_RGBA16 ? static_cast<const uint16_t *>(src)[p * 4 + 3] : static_cast<const uint8_t *>(src)[p * 4 + 3];
}

// FMT: CE_PIXEL_RGBA8 / RGBA16; Pixel: what k_tagged takes.  k_tagged's layout: a thread converts one group of four pixels
// once, then for every background blends the twelve values and stores 48 bytes into that background's slot - store12 chooses
// its width per slot, since slot k of an image whose pixel count is no multiple of 4 is not 16-byte aligned; the last
// n_pixels % 4 pixels go sample by sample, one pixel to a thread of block 0.
template <int FMT, class Pixel>
__global__ __launch_bounds__(kCicpBlock) void k_tagged_over(const Pixel px, const over_args ov)
{
    static_assert(FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16, "a format with alpha");
    const cicp_args &a = px.frame();
    const size_t n_groups = a.n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        uint32_t s[16];  // the group's samples, in memory order
        cicp_load_group<FMT>(a.src, tid, s);
        float v[12], t[4], u[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float c[3];
            px(s[4 * p], s[4 * p + 1], s[4 * p + 2], c);
            v[3 * p] = c[0], v[3 * p + 1] = c[1], v[3 * p + 2] = c[2];
            const uint32_t al = s[4 * p + 3];
            t[p] = ov.atab[al < a.maxv ? al : a.maxv];
            u[p] = 1.0f - t[p];
        }
        for (uint32_t k = 0; k < ov.n_bg; k++) {
            const float b0 = ov.bg[k][0], b1 = ov.bg[k][1], b2 = ov.bg[k][2];
            float o[12];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                o[3 * p] = over_blend(v[3 * p], b0, t[p], u[p]);
                o[3 * p + 1] = over_blend(v[3 * p + 1], b1, t[p], u[p]);
                o[3 * p + 2] = over_blend(v[3 * p + 2], b2, t[p], u[p]);
            }
            store12(a.dst + k * ov.slot_floats + tid * 12, o);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < a.n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        uint32_t c[3];
        cicp_load_pixel<FMT>(a.src, p, c);
        float v[3];
        px(c[0], c[1], c[2], v);
        const uint32_t al = over_load_alpha<FMT>(a.src, p);
        const float t = ov.atab[al < a.maxv ? al : a.maxv];
        const float u = 1.0f - t;
        for (uint32_t k = 0; k < ov.n_bg; k++) {
            float *d = a.dst + k * ov.slot_floats + p * 3;
#pragma unroll
            for (int i = 0; i < 3; i++) d[i] = over_blend(v[i], ov.bg[k][i], t, u);
        }
    }
}

// CE_PIXEL_RGBA_F32: n_pixels pixels of four floats at src (16-byte aligned staging), linear light already.  One 16-byte load
// per pixel, four pixels to a thread, and k_tagged_over's stores.  PREMUL: the colour samples hold colour * coverage.
template <bool PREMUL>
__global__ __launch_bounds__(kCicpBlock) void k_linear_over(const float *__restrict__ src, float *__restrict__ dst, size_t n_pixels, const over_args ov)
{
    const size_t n_groups = n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        float v[12], t[4], u[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const float4 q = reinterpret_cast<const float4 *>(src)[tid * 4 + p];
            v[3 * p] = linear_clamp(q.x), v[3 * p + 1] = linear_clamp(q.y), v[3 * p + 2] = linear_clamp(q.z);
            t[p] = over_coverage(q.w);
            u[p] = 1.0f - t[p];
        }
        for (uint32_t k = 0; k < ov.n_bg; k++) {
            const float b0 = ov.bg[k][0], b1 = ov.bg[k][1], b2 = ov.bg[k][2];
            float o[12];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if constexpr (PREMUL) {
                    o[3 * p] = over_blend_premul(v[3 * p], b0, u[p]);
                    o[3 * p + 1] = over_blend_premul(v[3 * p + 1], b1, u[p]);
                    o[3 * p + 2] = over_blend_premul(v[3 * p + 2], b2, u[p]);
                } else {
                    o[3 * p] = over_blend(v[3 * p], b0, t[p], u[p]);
                    o[3 * p + 1] = over_blend(v[3 * p + 1], b1, t[p], u[p]);
                    o[3 * p + 2] = over_blend(v[3 * p + 2], b2, t[p], u[p]);
                }
            }
            store12(dst + k * ov.slot_floats + tid * 12, o);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        const float4 q = reinterpret_cast<const float4 *>(src)[p];
        const float v[3] = {linear_clamp(q.x), linear_clamp(q.y), linear_clamp(q.z)};
        const float t = over_coverage(q.w);
        const float u = 1.0f - t;
        for (uint32_t k = 0; k < ov.n_bg; k++) {
            float *d = dst + k * ov.slot_floats + p * 3;
#pragma unroll
            for (int i = 0; i < 3; i++) d[i] = PREMUL ? over_blend_premul(v[i], ov.bg[k][i], u) : over_blend(v[i], ov.bg[k][i], t, u);
        }
    }
}

}  // namespace
