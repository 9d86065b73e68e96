// The device code of the Delta E ITP maps (hdr_fidelity.hip: k_delta_e_itp_map; include/ce_metrics.h: ce_batch_delta_e_itp_map;
// DESIGN.md section 20), kept under hdr_fidelity_kernel.h's rules - beside the HIP keywords, float4 and blockIdx / threadIdx /
// gridDim it uses uint4 for its 16-byte store and atomicMax(uint32_t *, uint32_t) for a cell's maximum - so that
// tests/cpp/delta_e_itp_map_kernel_host.cpp can compile the same text for the host.  hdrf_map_lane is k_hdr_fidelity's
// hdrf_lane - the same frame, the same loads, the same searches (hdrf_diffs) and the same Delta E (hdrf_itp_q20) - with other
// ends for a pixel's k: a store, a cell's maximum, eight comparisons.  Only the L, M, S differences are used, so the compiler
// drops the three searches a side that the R, G, B codes would cost.
#pragma once

#include "hdr_fidelity_kernel.h"

namespace {

constexpr int kItpMaxThresholds = 8;  // CE_DELTA_E_ITP_MAX_THRESHOLDS

struct hdrf_map_args {
    uint32_t *map;       // nullptr: counts only.  lb = 0: [pair][n_pixels], written whole.  lb > 0: [pair][ch][cw], zeroed before the launch
    uint32_t w;          // the image's width; n_pixels = w * h
    uint32_t lb;         // log2 of the cell's side B: 0 .. 6
    uint32_t cw;         // cells a row, ceil(w / B)
    size_t pair_len;     // elements of a pair's map: n_pixels, or ch * cw
    uint32_t thr[kItpMaxThresholds];  // the caller's thresholds, padded with 2^32 - 1, which nothing exceeds
};

// k saturated to the map's 32 bits
__device__ __forceinline__ uint32_t hdrf_map_value(unsigned long long k) { return k > 0xffffffffull ? 0xffffffffu : (uint32_t)k; }

template <int DEPTH>
__device__ __forceinline__ uint32_t hdrf_map_pixel(const hdrf_args &a, const hdrf_map_args &m, const float *s_tab, const float ref[3],
                                                   const float test[3], uint32_t cnt[kItpMaxThresholds])
{
    long long d[6];
    hdrf_diffs<DEPTH>(a, s_tab, ref, test, d);
    const uint32_t v = hdrf_map_value(hdrf_itp_q20(a, d));
#pragma unroll
    for (int j = 0; j < kItpMaxThresholds; j++) cnt[j] += v > m.thr[j] ? 1u : 0u;
    return v;
}

// The maxima of cells (lb > 0), for the pixels a lane meets in raster order: the lane keeps the maximum of the run of pixels
// that fall into one cell and hands it over when the cell changes - once per four-pixel group when w is a multiple of four.
// The cell array starts at zero and only ever takes maxima, so a run whose maximum is 0 has nothing to hand over.
struct hdrf_cell_run {
    size_t cell;
    uint32_t best;
};
__device__ __forceinline__ void hdrf_cell_flush(uint32_t *cells, const hdrf_cell_run &r)
{
    if (r.best) atomicMax(cells + r.cell, r.best);
}
__device__ __forceinline__ void hdrf_cell_put(uint32_t *cells, hdrf_cell_run &r, size_t cell, uint32_t v)
{
    if (cell != r.cell) {
        hdrf_cell_flush(cells, r);
        r.cell = cell, r.best = 0;
    }
    r.best = v > r.best ? v : r.best;
}

// After the barrier: this lane's share of pair first + blockIdx.y in hdrf_lane's frame.  cnt[j] = how many of its pixels exceed
// thr[j].  A pair's map starts 16-byte aligned on the wide path: pair_len = n_pixels is a multiple of four there.
template <int DEPTH>
__device__ __forceinline__ void hdrf_map_lane(const hdrf_args &a, const hdrf_map_args &m, const float *s_tab, uint32_t cnt[kItpMaxThresholds])
{
    const uint32_t p = hdrf_pair(a);
    const size_t img = a.n_pixels * 3;
    const float *ref = a.refs + (size_t)a.pair_ref[p] * img;
    const float *test = a.tests + (size_t)p * img;
    uint32_t *map = m.map ? m.map + (size_t)p * m.pair_len : nullptr;
    const size_t tid = (size_t)blockIdx.x * kHdrfThreads + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * kHdrfThreads;
#pragma unroll
    for (int j = 0; j < kItpMaxThresholds; j++) cnt[j] = 0;
    const bool cells = map && m.lb;
    hdrf_cell_run run{0, 0};
    if ((a.n_pixels & 3) == 0) {
        const float4 *r4 = reinterpret_cast<const float4 *>(ref);
        const float4 *t4 = reinterpret_cast<const float4 *>(test);
        for (size_t i = tid; i < a.n_pixels / 4; i += nthreads) {
            const float4 r0 = r4[i * 3], r1 = r4[i * 3 + 1], r2 = r4[i * 3 + 2];
            const float4 t0 = t4[i * 3], t1 = t4[i * 3 + 1], t2 = t4[i * 3 + 2];
            const float r[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
            const float t[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = hdrf_map_pixel<DEPTH>(a, m, s_tab, r + 3 * k, t + 3 * k, cnt);
            if (cells) {
                size_t y = (i * 4) / m.w;
                uint32_t x = (uint32_t)((i * 4) - y * m.w);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    hdrf_cell_put(map, run, (y >> m.lb) * m.cw + (x >> m.lb), v[k]);
                    if (++x == m.w) x = 0, y++;
                }
            } else if (map) {
                uint4 o;
                o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
                reinterpret_cast<uint4 *>(map)[i] = o;
            }
        }
    } else {
        for (size_t i = tid; i < a.n_pixels; i += nthreads) {
            const float r[3] = {ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2]};
            const float t[3] = {test[i * 3], test[i * 3 + 1], test[i * 3 + 2]};
            const uint32_t v = hdrf_map_pixel<DEPTH>(a, m, s_tab, r, t, cnt);
            if (cells) {
                const size_t y = i / m.w;
                const uint32_t x = (uint32_t)(i - y * m.w);
                hdrf_cell_put(map, run, (y >> m.lb) * m.cw + (x >> m.lb), v);
            } else if (map) {
                map[i] = v;
            }
        }
    }
    if (cells) hdrf_cell_flush(map, run);
}

}  // namespace
