// The device code of the HLG ingest (hlg.hip), kept like cicp_kernel.h, whose frame it is, free of anything but the HIP
// keywords, uint2 / uint4 / float4 and blockIdx / threadIdx, so that tests/cpp/hlg_kernel_host.cpp can compile the same text
// for the host and run it under the host sanitizers.  Every f32 and every f64 product and sum is a separately rounded
// operation: this text is compiled with -ffp-contract=off on the device and on the host (include/ce_metrics.h: the
// definition of ce_batch_set_*_hlg).
#pragma once

#include "cicp_kernel.h"
#include "hlg_pixel.h"

namespace {

// k_cicp with hlg_pixel in cicp_pixel's place: FMT, the group of four pixels from aligned loads, store12's choice between
// 16- and 4-byte stores, and the n_pixels % 4 tail in block 0 are its.  The table stays in global memory at every depth.
template <int FMT, bool MATRIX>
__global__ __launch_bounds__(kCicpBlock) void k_hlg(const hlg_args a)
{
    constexpr int NC = (FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16) ? 4 : 3;
    const size_t n_groups = a.c.n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        uint32_t s[4 * NC];  // the group's samples, in memory order
        cicp_load_group<FMT>(a.c.src, tid, s);
        float o[12];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float px[3];
            hlg_pixel<MATRIX>(a, s[NC * p], s[NC * p + 1], s[NC * p + 2], px);
            o[3 * p] = px[0], o[3 * p + 1] = px[1], o[3 * p + 2] = px[2];
        }
        store12(a.c.dst + tid * 12, o);
    }
    if (blockIdx.x == 0 && threadIdx.x < a.c.n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        uint32_t v[3];
        cicp_load_pixel<FMT>(a.c.src, p, v);
        float px[3];
        hlg_pixel<MATRIX>(a, v[0], v[1], v[2], px);
#pragma unroll
        for (int c = 0; c < 3; c++) a.c.dst[p * 3 + c] = px[c];
    }
}

}  // namespace
