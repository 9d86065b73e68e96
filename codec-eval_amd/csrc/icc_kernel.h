// The device code of the ICC ingest into integer slots (include/ce_metrics.h: the matrix/TRC definition, step 4), kept as free
// of HIP as cicp_kernel.h, whose loads it shares, so that tests/cpp/icc_kernel_host.cpp compiles the same text for the host
// and runs it under the host sanitizers.  k_icc_encode is k_tagged's frame with another store: the pixel's three linear
// values each go through a search of the sRGB code thresholds and leave as u8 or u16 samples.  The thresholds are gathered
// from global memory at every depth, like the pixel's tables: 1 KB at depth 8, which stays in the vector L1, to 256 KB at
// depth 16, which stays in L2; no LDS.  Compiled with -ffp-contract=off on the device and on the host.
#pragma once

#include "cicp_kernel.h"
#include "icc_pixel.h"

namespace {

// two dwords stored as one 8-byte access
struct alignas(8) icc_dword_pair {
    uint32_t lo, hi;
};

// code = #{ k in 1 .. 2 * top - 1 : x >= thr[k] } for strictly increasing thr[1 ..]: log2(top) + 1 steps, each one gather and
// one conditional add, the same for every lane; NaN compares false at every step and gives 0.  thr[0] is never read.
__device__ __forceinline__ uint32_t icc_encode(const float *__restrict__ thr, uint32_t top, float x)
{
    uint32_t pos = 0;
    for (uint32_t step = top; step != 0; step >>= 1) pos += x >= thr[pos + step] ? step : 0u;
    return pos;
}

// FMT and Pixel as k_tagged's (the pixel's frame() holds src and n_pixels; its dst is not read); dst: the slot, packed u8 RGB
// or with OUT16 packed u16 RGB; thr: thr[1 .. 2^D - 1] the thresholds of the slot's depth D; top = 2^(D - 1).  A thread
// converts one group of four pixels and stores its 12 bytes as three dwords where the slot is 4-byte aligned, its 24 bytes
// as three 8-byte pairs where the slot is 8-byte aligned, and sample by sample otherwise - the same choice for every thread
// of a launch, since a group starts a multiple of 12 or 24 bytes into its slot.  The last n_pixels % 4 pixels go sample by
// sample, one pixel to a thread of block 0.
template <int FMT, bool OUT16, class Pixel>
__global__ __launch_bounds__(kCicpBlock) void k_icc_encode(const Pixel px, void *dst, const float *__restrict__ thr, uint32_t top)
{
    constexpr int NC = (FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16) ? 4 : 3;
    const cicp_args &a = px.frame();
    const size_t n_groups = a.n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        uint32_t s[4 * NC];  // the group's samples, in memory order
        cicp_load_group<FMT>(a.src, tid, s);
        float x[12];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float v[3];
            px(s[NC * p], s[NC * p + 1], s[NC * p + 2], v);
            x[3 * p] = v[0], x[3 * p + 1] = v[1], x[3 * p + 2] = v[2];
        }
        // icc_encode on the twelve values side by side: a step's twelve gathers do not depend on each other
        uint32_t c[12] = {};
        for (uint32_t step = top; step != 0; step >>= 1) {
#pragma unroll
            for (int i = 0; i < 12; i++) c[i] += x[i] >= thr[c[i] + step] ? step : 0u;
        }
        if constexpr (OUT16) {
            uint16_t *p = static_cast<uint16_t *>(dst) + tid * 12;
            if ((reinterpret_cast<uintptr_t>(p) & 7) == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++)
                    reinterpret_cast<icc_dword_pair *>(p)[i] = icc_dword_pair{c[4 * i] | (c[4 * i + 1] << 16), c[4 * i + 2] | (c[4 * i + 3] << 16)};
            } else {
#pragma unroll
                for (int i = 0; i < 12; i++) p[i] = (uint16_t)c[i];
            }
        } else {
            uint8_t *p = static_cast<uint8_t *>(dst) + tid * 12;
            if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++)
                    reinterpret_cast<uint32_t *>(p)[i] = c[4 * i] | (c[4 * i + 1] << 8) | (c[4 * i + 2] << 16) | (c[4 * i + 3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 12; i++) p[i] = (uint8_t)c[i];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < a.n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        uint32_t v[3];
        cicp_load_pixel<FMT>(a.src, p, v);
        float o[3];
        px(v[0], v[1], v[2], o);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t code = icc_encode(thr, top, o[k]);
            if constexpr (OUT16) static_cast<uint16_t *>(dst)[p * 3 + k] = (uint16_t)code;
            else static_cast<uint8_t *>(dst)[p * 3 + k] = (uint8_t)code;
        }
    }
}

}  // namespace
