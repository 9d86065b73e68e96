// The device code of the CIEDE2000 maps (ciede2000_map.hip: k_ciede2000_map; include/ce_metrics.h: ce_batch_ciede2000_map;
// DESIGN.md section 34), kept under ciede2000_kernel.h's rules - beside the HIP keywords, uint4 and blockIdx / threadIdx /
// gridDim it uses atomicMax(uint32_t *, uint32_t) for a cell's maximum - so that tests/cpp/ciede2000_map_kernel_host.cpp can
// compile the same text for the host.  cie_map_lane is k_ciede2000's cie_lane - the same staging (cie_stage), the same tables
// (cie_tabs, cie_lookup), the same wide and scalar loads, the same skip of equal code triples and the same pixel
// (ciede2000_pixel.h: cie_lab_of, cie_de2000_terms, cie_terms_q20) - with other ends for a pixel's value: a store, a cell's
// maximum, eight comparisons.  cie_args::pair_ref and ::tests start at the call's first pair; ::thr are the call's thresholds.
#pragma once

#include "ciede2000_kernel.h"

namespace {

constexpr uint32_t kCieMapDe = 0, kCieMapDl = 1, kCieMapDc = 2, kCieMapDh = 3;  // CE_CIEDE2000_MAP_DE, _DL, _DC, _DH

struct cie_map_args {
    uint32_t *map;    // nullptr: counts only.  lb = 0: [pair][n_pixels], written whole.  lb > 0: [pair][ch][cw], zeroed before the launch
    uint32_t what;    // kCieMap*: which of the pixel's four values
    uint32_t w;       // the image's width; n_pixels = w * h
    uint32_t lb;      // log2 of the cell's side B: 0 .. 6
    uint32_t cw;      // cells a row, ceil(w / B)
    size_t pair_len;  // elements of a pair's map: n_pixels, or ch * cw
};

// rint(|x| 2^20): the magnitude of a term in q's unit.  |x| clears the sign bit, so -0 gives 0; a term stays under 110
// (include/ce_metrics.h), so the integer is under 2^27.
__device__ __forceinline__ uint32_t cie_term_q20(double x)
{
    return (uint32_t)(unsigned long long)__builtin_rint(__builtin_fabs(x) * 1048576.0);
}

// one pixel of a pair -> the value `what` selects, counted against the thresholds.  Two equal code triples at one depth are
// two equal Lab values: dL = 0, dC = 0 and dH is a multiple of sin_deg(0) = 0, so all four values are 0, nothing exceeds a
// threshold, and the arithmetic is skipped as in cie_pixel.
__device__ __forceinline__ uint32_t cie_map_pixel(const cie_args &a, const cie_map_args &m, const cie_tab &tr, const cie_tab &tt,
                                                  const uint32_t r[3], const uint32_t t[3], uint32_t cnt[kCieMaxThresholds])
{
    if (a.depth[0] == a.depth[1] && r[0] == t[0] && r[1] == t[1] && r[2] == t[2]) return 0u;
    const cie_lab p1 = cie_lab_of(cie_lookup(tr, r[0]), cie_lookup(tr, r[1]), cie_lookup(tr, r[2]));
    const cie_lab p2 = cie_lab_of(cie_lookup(tt, t[0]), cie_lookup(tt, t[1]), cie_lookup(tt, t[2]));
    const cie_terms e = cie_de2000_terms(p1, p2);
    const uint32_t v = m.what == kCieMapDe ? cie_terms_q20(e) : cie_term_q20(m.what == kCieMapDl ? e.tl : m.what == kCieMapDc ? e.tc : e.th);
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) cnt[j] += v > a.thr[j] ? 1u : 0u;
    return v;
}

// The maxima of cells (lb > 0), for the pixels a lane meets in raster order, as hdrf_cell_run (hdr_fidelity_map_kernel.h): the
// lane keeps the maximum of the run of pixels that fall into one cell and hands it over when the cell changes.  The cell array
// starts at zero and only ever takes maxima, so a run whose maximum is 0 has nothing to hand over.  A lane's unit of 16 or 8
// pixels changes cell inside the unit wherever B is below the unit, at a row's end wherever w is no multiple of the unit, and
// spans several rows where w is below it; every pixel therefore names its own cell.
struct cie_cell_run {
    size_t cell;
    uint32_t best;
};
__device__ __forceinline__ void cie_cell_flush(uint32_t *cells, const cie_cell_run &r)
{
    if (r.best) atomicMax(cells + r.cell, r.best);
}
__device__ __forceinline__ void cie_cell_put(uint32_t *cells, cie_cell_run &r, size_t cell, uint32_t v)
{
    if (cell != r.cell) {
        cie_cell_flush(cells, r);
        r.cell = cell, r.best = 0;
    }
    r.best = v > r.best ? v : r.best;
}

// After the barrier: this lane's share of pair first + blockIdx.y in cie_lane's frame.  cnt[j] = how many of its pixels exceed
// thr[j].  On the wide path a lane's unit of 16 or 8 pixels owns 64 or 32 contiguous bytes of a block-1 map, which start 16-byte
// aligned (pair_len = n_pixels is a multiple of the unit there): the pixel loop stays rolled and indexes no register by a
// variable, so the values pass through a window of four dwords that is shifted down by one per pixel - as the input dwords
// are - and stored whole after every fourth.
template <bool DEEP>
__device__ __forceinline__ void cie_map_lane(const cie_args &a, const cie_map_args &m, const float *s_tab, uint32_t cnt[kCieMaxThresholds])
{
    cie_tab tr, tt;
    cie_tabs(a, s_tab, tr, tt);
    const uint32_t p = cie_pair(a);
    const size_t img = a.n_pixels * 3 * (DEEP ? 2 : 1);  // bytes
    const uint8_t *ref = static_cast<const uint8_t *>(a.refs) + (size_t)a.pair_ref[p] * img;
    const uint8_t *test = static_cast<const uint8_t *>(a.tests) + (size_t)p * img;
    uint32_t *map = m.map ? m.map + (size_t)p * m.pair_len : nullptr;
    const size_t tid = (size_t)blockIdx.x * kCieThreads + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * kCieThreads;
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) cnt[j] = 0;
    const bool cells = map && m.lb;
    cie_cell_run run{0, 0};
    if (cie_wide(a.n_pixels, DEEP)) {
        const uint4 *r4 = reinterpret_cast<const uint4 *>(ref);
        const uint4 *t4 = reinterpret_cast<const uint4 *>(test);
        for (size_t i = tid; i < a.n_pixels / cie_unit(DEEP); i += nthreads) {
            const uint4 r0 = r4[i * 3], r1 = r4[i * 3 + 1], r2 = r4[i * 3 + 2];
            const uint4 t0 = t4[i * 3], t1 = t4[i * 3 + 1], t2 = t4[i * 3 + 2];
            uint32_t rw[14] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, 0u, 0u};
            uint32_t tw[14] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, 0u, 0u};
            size_t y = 0;
            uint32_t x = 0;
            if (cells) {
                y = (i * cie_unit(DEEP)) / m.w;
                x = (uint32_t)((i * cie_unit(DEEP)) - y * m.w);
            }
            uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;  // the last four values, oldest first
            uint4 *out4 = cells || !map ? nullptr : reinterpret_cast<uint4 *>(map + i * cie_unit(DEEP));
#pragma unroll 1
            for (uint32_t k = 0; k < cie_unit(DEEP); k++) {
                uint32_t r[3], t[3];
                if (DEEP) {
                    r[0] = rw[0] & 0xffffu, r[1] = rw[0] >> 16, r[2] = rw[1] & 0xffffu;
                    t[0] = tw[0] & 0xffffu, t[1] = tw[0] >> 16, t[2] = tw[1] & 0xffffu;
                } else {
                    r[0] = rw[0] & 0xffu, r[1] = (rw[0] >> 8) & 0xffu, r[2] = (rw[0] >> 16) & 0xffu;
                    t[0] = tw[0] & 0xffu, t[1] = (tw[0] >> 8) & 0xffu, t[2] = (tw[0] >> 16) & 0xffu;
                }
                const uint32_t v = cie_map_pixel(a, m, tr, tt, r, t, cnt);
                if (cells) {
                    cie_cell_put(map, run, (y >> m.lb) * m.cw + (x >> m.lb), v);
                    if (++x == m.w) x = 0, y++;
                } else if (map) {
                    o0 = o1, o1 = o2, o2 = o3, o3 = v;
                    if ((k & 3u) == 3u) {
                        uint4 o;
                        o.x = o0, o.y = o1, o.z = o2, o.w = o3;
                        out4[k >> 2] = o;
                    }
                }
#pragma unroll
                for (int j = 0; j < 12; j++) {
                    if (DEEP) {
                        rw[j] = (rw[j + 1] >> 16) | (rw[j + 2] << 16);
                        tw[j] = (tw[j + 1] >> 16) | (tw[j + 2] << 16);
                    } else {
                        rw[j] = (rw[j] >> 24) | (rw[j + 1] << 8);
                        tw[j] = (tw[j] >> 24) | (tw[j + 1] << 8);
                    }
                }
            }
        }
    } else {
        for (size_t i = tid; i < a.n_pixels; i += nthreads) {
            uint32_t r[3], t[3];
            if (DEEP) {
                const uint16_t *r16 = reinterpret_cast<const uint16_t *>(ref), *t16 = reinterpret_cast<const uint16_t *>(test);
                r[0] = r16[i * 3], r[1] = r16[i * 3 + 1], r[2] = r16[i * 3 + 2];
                t[0] = t16[i * 3], t[1] = t16[i * 3 + 1], t[2] = t16[i * 3 + 2];
            } else {
                r[0] = ref[i * 3], r[1] = ref[i * 3 + 1], r[2] = ref[i * 3 + 2];
                t[0] = test[i * 3], t[1] = test[i * 3 + 1], t[2] = test[i * 3 + 2];
            }
            const uint32_t v = cie_map_pixel(a, m, tr, tt, r, t, cnt);
            if (cells) {
                const size_t y = i / m.w;
                const uint32_t x = (uint32_t)(i - y * m.w);
                cie_cell_put(map, run, (y >> m.lb) * m.cw + (x >> m.lb), v);
            } else if (map) {
                map[i] = v;
            }
        }
    }
    if (cells) cie_cell_flush(map, run);
}

}  // namespace
