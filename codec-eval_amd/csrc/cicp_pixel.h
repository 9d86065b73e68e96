// One pixel of the CICP ingest: the arguments, the clamp of a linear image and the table gather with the separately rounded
// f32 matrix, apart from the kernels so that a file that needs the pixel does not emit them, and cicp_px, the pixel as the
// type that the two frames take (cicp_kernel.h: k_tagged; yuv_cicp_kernel.h: k_yuv_tagged).  hlg_pixel.h builds its pixel on
// the same arguments, matrix and clamp.  Host-compilable like the headers that include it, and compiled with
// -ffp-contract=off.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

namespace {

struct cicp_args {
    const void *src;     // packed RGB / RGBA, u8 or u16 samples, 16-byte aligned
    float *dst;          // the slot: packed f32 RGB, 4-byte aligned (16 where the slot's offset allows)
    size_t n_pixels;
    const float *table;  // maxv + 1 entries
    uint32_t maxv;
    float m[9];          // row-major; unused without MATRIX
};

// a linear image's sample: NaN -> 0, then the clamp to [-CE_LINEAR_MAX, CE_LINEAR_MAX]
__device__ __forceinline__ float linear_clamp(float v)
{
    if (v != v) return 0.0f;
    return v > CE_LINEAR_MAX ? CE_LINEAR_MAX : (v < -CE_LINEAR_MAX ? -CE_LINEAR_MAX : v);
}

// steps 3 and 4 of the definition on one pixel's three linear-light values: the separately rounded f32 3 x 3 for primaries
// other than 1, then the clamp of a linear image (shared with hlg_pixel.h, whose values are display light)
template <bool MATRIX>
__device__ __forceinline__ void cicp_matrix_clamp(const cicp_args &a, float tr, float tg, float tb, float (&o)[3])
{
    if constexpr (MATRIX) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float p0 = a.m[3 * i] * tr, p1 = a.m[3 * i + 1] * tg, p2 = a.m[3 * i + 2] * tb;
            const float s01 = p0 + p1;
            o[i] = linear_clamp(s01 + p2);
        }
    } else {
        o[0] = linear_clamp(tr), o[1] = linear_clamp(tg), o[2] = linear_clamp(tb);
    }
}

template <bool MATRIX>
__device__ __forceinline__ void cicp_pixel(const cicp_args &a, uint32_t r, uint32_t g, uint32_t b, float (&o)[3])
{
    const float tr = a.table[r < a.maxv ? r : a.maxv], tg = a.table[g < a.maxv ? g : a.maxv], tb = a.table[b < a.maxv ? b : a.maxv];
    cicp_matrix_clamp<MATRIX>(a, tr, tg, tb, o);
}

// What a frame is given as its pixel: the arguments by value, the fields the frames themselves read (src, dst, n_pixels)
// and the conversion of one pixel's three code values.  MATRIX: primaries other than 1.
template <bool MATRIX>
struct cicp_px {
    cicp_args a;
    __device__ __forceinline__ const cicp_args &frame() const { return a; }
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t g, uint32_t b, float (&o)[3]) const { cicp_pixel<MATRIX>(a, r, g, b, o); }
};

}  // namespace
