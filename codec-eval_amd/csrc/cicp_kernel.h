// The device code of the ingest of packed code values into a linear batch - CICP and HLG - and of the linear-f32 upload
// (cicp.hip), kept free of anything but the HIP keywords, uint2 / uint4 / float4 and blockIdx / threadIdx, so that
// tests/cpp/cicp_kernel_host.cpp and hlg_kernel_host.cpp can compile the same text for the host - thread and block indices as
// loop variables - and run it under the host sanitizers against a source and a slot allocated at exactly their size.  One
// frame, k_tagged, with the pixel as a parameter: cicp_pixel.h's cicp_px or hlg_pixel.h's hlg_px.  Every f32 and every f64
// product and sum is a separately rounded operation: this text is compiled with -ffp-contract=off on the device and on the
// host, and its expressions are written so that no other evaluation order is allowed (include/ce_metrics.h: the definitions
// of ce_batch_set_*_cicp and ce_batch_set_*_hlg).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

#include "cicp_pixel.h"

namespace {

constexpr int kCicpBlock = 256;  // threads per block; a thread owns 4 pixels: a 768 x 512 image is 384 blocks

// 12 floats (four pixels) to p: three 16-byte stores where the address allows, twelve 4-byte stores otherwise; the same
// choice for every thread of a launch, since a group starts a multiple of 48 bytes into its slot
__device__ __forceinline__ void store12(float *p, const float (&o)[12])
{
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) reinterpret_cast<float4 *>(p)[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) p[i] = o[i];
    }
}

// The samples of group `tid` (four pixels) of a packed FMT image at src, in memory order, from aligned loads (12 bytes: three
// dwords; 16: one uint4; 24: three uint2; 32: two uint4).
template <int FMT>
__device__ __forceinline__ void cicp_load_group(const void *src, size_t tid,
                                                uint32_t (&s)[4 * ((FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16) ? 4 : 3)])
{
    constexpr bool S16 = FMT == CE_PIXEL_RGB16 || FMT == CE_PIXEL_RGBA16, ALPHA = FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16;
    constexpr int NC = ALPHA ? 4 : 3;
    if constexpr (!S16) {
        uint32_t d[NC];
        if constexpr (ALPHA) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[tid];
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[NC - 1] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < NC; i++) d[i] = reinterpret_cast<const uint32_t *>(src)[tid * NC + i];
        }
#pragma unroll
        for (int i = 0; i < 4 * NC; i++) s[i] = (d[i / 4] >> (8 * (i % 4))) & 255u;
    } else {
        uint32_t d[2 * NC];
        if constexpr (ALPHA) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const uint4 v = reinterpret_cast<const uint4 *>(src)[tid * 2 + i];
                d[4 * i] = v.x, d[4 * i + 1] = v.y, d[4 * i + 2] = v.z, d[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const uint2 v = reinterpret_cast<const uint2 *>(src)[tid * 3 + i];
                d[2 * i] = v.x, d[2 * i + 1] = v.y;
            }
        }
#pragma unroll
        for (int i = 0; i < 4 * NC; i++) s[i] = (d[i / 2] >> (16 * (i % 2))) & 0xffffu;
    }
}

// the three colour samples of pixel p, sample by sample (the tail)
template <int FMT>
__device__ __forceinline__ void cicp_load_pixel(const void *src, size_t p, uint32_t (&v)[3])
{
    constexpr bool S16 = FMT == CE_PIXEL_RGB16 || FMT == CE_PIXEL_RGBA16, ALPHA = FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16;
    constexpr int NC = ALPHA ? 4 : 3;
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = S16 ? static_cast<const uint16_t *>(src)[p * NC + c] : static_cast<const uint8_t *>(src)[p * NC + c];
}

// FMT: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 (alpha dropped); Pixel: cicp_px<MATRIX> or hlg_px<MATRIX>, whose frame() holds
// src, dst and n_pixels.  A thread converts one group of four pixels from the registers its aligned loads filled and stores
// 48 bytes; the last n_pixels % 4 pixels go sample by sample, one pixel to a thread of block 0.  Either pixel gathers its
// table from global memory at every depth: 1, 4 and 16 KB stay in the vector L1 and the 256 KB of depth 16 in L2, one code
// path.
template <int FMT, class Pixel>
__global__ __launch_bounds__(kCicpBlock) void k_tagged(const Pixel px)
{
    constexpr int NC = (FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16) ? 4 : 3;
    const cicp_args &a = px.frame();
    const size_t n_groups = a.n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        uint32_t s[4 * NC];  // the group's samples, in memory order
        cicp_load_group<FMT>(a.src, tid, s);
        float o[12];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float v[3];
            px(s[NC * p], s[NC * p + 1], s[NC * p + 2], v);
            o[3 * p] = v[0], o[3 * p + 1] = v[1], o[3 * p + 2] = v[2];
        }
        store12(a.dst + tid * 12, o);
    }
    if (blockIdx.x == 0 && threadIdx.x < a.n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        uint32_t v[3];
        cicp_load_pixel<FMT>(a.src, p, v);
        float o[3];
        px(v[0], v[1], v[2], o);
#pragma unroll
        for (int c = 0; c < 3; c++) a.dst[p * 3 + c] = o[c];
    }
}

// The CE_PIXEL_RGB_F32 upload: n_samples floats from 16-byte aligned staging into the slot through linear_clamp, four to a
// thread (one 16-byte load; one 16-byte store where the slot's address allows), the last n_samples % 4 one to a thread of
// block 0.
__global__ __launch_bounds__(kCicpBlock) void k_linear_sanitise(const float *__restrict__ src, float *__restrict__ dst, size_t n_samples)
{
    const size_t n_groups = n_samples / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        const float4 v = reinterpret_cast<const float4 *>(src)[tid];
        const float o0 = linear_clamp(v.x), o1 = linear_clamp(v.y), o2 = linear_clamp(v.z), o3 = linear_clamp(v.w);
        float *p = dst + tid * 4;
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0)
            *reinterpret_cast<float4 *>(p) = make_float4(o0, o1, o2, o3);
        else
            p[0] = o0, p[1] = o1, p[2] = o2, p[3] = o3;
    }
    if (blockIdx.x == 0 && threadIdx.x < n_samples % 4) {
        const size_t i = n_groups * 4 + threadIdx.x;
        dst[i] = linear_clamp(src[i]);
    }
}

}  // namespace
