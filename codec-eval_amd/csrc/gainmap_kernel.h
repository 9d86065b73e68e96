// The device code of the gain-map ingest (gainmap.hip), kept as free of HIP as cicp_kernel.h, whose loads and stores it
// uses, so that tests/cpp/gainmap_kernel_host.cpp can compile the same text for the host and run it under the host
// sanitizers against a base, a map, tables and a slot allocated at exactly their size.  k_tagged's pixel sees three code
// values and no position; a gain-map pixel samples the map around its own centre, so this is a frame of its own,
// k_gainmap, of the same shape.  Every f32 and f64 operation is rounded separately: compiled with -ffp-contract=off on the
// device and on the host (include/ce_metrics.h: the definition of ce_batch_set_*_gainmap).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ce_metrics.h"

#include "cicp_kernel.h"
#include "gainmap_pixel.h"

namespace {

// FMT: CE_PIXEL_RGB8 / RGBA8 / RGB16 / RGBA16 (alpha dropped); NCH: the map's channels, 1 or 3; MATRIX: primaries other than
// 1.  As in k_tagged a thread converts one group of four consecutive pixels - consecutive by linear index, so a group may
// straddle a row end, or with w < 4 several: (x, y) is divided out once for the group's first pixel and stepped from there -
// from the registers its aligned loads filled, and stores 48 bytes; the last n_pixels % 4 pixels go sample by sample, one
// pixel to a thread of block 0.  The map's four neighbours and the log2-gain table (2 or 6 KB of doubles) are gathered from
// global memory: the table stays in the vector L1 like the transfer tables, and a map is at most the base's size and usually
// a sixteenth of it, each sample read by the many pixels around it.
template <int FMT, int NCH, bool MATRIX>
__global__ __launch_bounds__(kCicpBlock) void k_gainmap(const gainmap_args a)
{
    constexpr int NC = (FMT == CE_PIXEL_RGBA8 || FMT == CE_PIXEL_RGBA16) ? 4 : 3;
    const size_t n_groups = a.c.n_pixels / 4;
    const size_t tid = (size_t)blockIdx.x * kCicpBlock + threadIdx.x;
    if (tid < n_groups) {
        uint32_t s[4 * NC];  // the group's samples, in memory order
        cicp_load_group<FMT>(a.c.src, tid, s);
        uint32_t y = (uint32_t)(tid * 4 / a.w), x = (uint32_t)(tid * 4 - (size_t)y * a.w);
        float o[12];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float v[3];
            gainmap_pixel<NCH, MATRIX>(a, x, y, s[NC * p], s[NC * p + 1], s[NC * p + 2], v);
            o[3 * p] = v[0], o[3 * p + 1] = v[1], o[3 * p + 2] = v[2];
            if (++x == a.w) x = 0, y++;
        }
        store12(a.c.dst + tid * 12, o);
    }
    if (blockIdx.x == 0 && threadIdx.x < a.c.n_pixels % 4) {
        const size_t p = n_groups * 4 + threadIdx.x;
        uint32_t v[3];
        cicp_load_pixel<FMT>(a.c.src, p, v);
        float o[3];
        gainmap_pixel<NCH, MATRIX>(a, (uint32_t)(p % a.w), (uint32_t)(p / a.w), v[0], v[1], v[2], o);
#pragma unroll
        for (int c = 0; c < 3; c++) a.c.dst[p * 3 + c] = o[c];
    }
}

}  // namespace
