// The device code of the SSIM / MS-SSIM maps (msssim_map.hip: k_msssim_level_map; include/ce_metrics.h: ce_batch_msssim_map;
// DESIGN.md section 29), kept under msssim_kernel.h's rules - beside the HIP keywords and blockIdx / threadIdx / gridDim it uses
// atomicMax(uint32_t *, uint32_t) for the cells that span tiles, as hdr_fidelity_map_kernel.h does - so that
// tests/cpp/msssim_map_kernel_host.cpp can compile the same text for the host.  The map kernel is k_msssim_level with other
// ends for a position's integers: mss_stage, mss_columns, mss_rows and mss_position are the score kernel's own, so a map
// value is 2^32 minus exactly the integer the score summed.  It is split at its barriers like the score kernel: after
// mss_columns' barrier mss_map_lane forms the lane's two values, counts them against the thresholds, stores them (block 1)
// or parks the larger in LDS (cells); then mss_map_rows reduces along the rows of the tile and mss_map_cells down its
// columns, each behind a barrier.  The reduction of the counts across lanes stays in msssim_map.hip.
#pragma once

#include "msssim_kernel.h"

namespace {

constexpr int kMssMapMaxThresholds = 8;  // CE_MSSSIM_MAP_MAX_THRESHOLDS
constexpr int kMssPairsW = kMssTileW / 2;  // lanes a row of the tile: each parks the larger of its two values
constexpr int kMssParkLen = kMssPairsW * kMssTileH;

struct alignas(8) mss_u2 {
    uint32_t a, b;
};

// The valid region of the level is vw x vh = (w - 10) x (h - 10); blockIdx.y / 3 is the pair's place in `map` and in the counts.
struct mss_map_args {
    uint32_t *map;   // nullptr: counts only.  lb = 0: [pair][3][vh][vw], written whole.  lb = 1 .. 4: [pair][3][ch][cw], written
                     // whole, a cell by one block.  lb = 5, 6: the same, zeroed before the launch
    uint32_t what;   // 0: qs, 1: qc
    uint32_t lb;     // log2 of the cell's side B: 0 .. 6
    uint32_t cw, ch; // cells a row and a column: ceil(vw / B), ceil(vh / B)
    uint32_t thr[kMssMapMaxThresholds];  // the caller's thresholds, padded with 2^32 - 1, which nothing exceeds
};

// the dissimilarity 2^32 - q saturated to the map's 32 bits: 0 for q >= 2^32, 2^32 - 1 for q <= 1
__device__ __forceinline__ uint32_t mss_map_value(long long q)
{
    const long long d = 4294967296ll - q;
    return d < 0 ? 0u : d > 0xffffffffll ? 0xffffffffu : (uint32_t)d;
}

__device__ __forceinline__ uint32_t mss_map_position(const mss_args &a, const mss_map_args &m, const double f[kMssStreams],
                                                     uint32_t cnt[kMssMapMaxThresholds])
{
    long long q[2];
    mss_position(a, f, q);
    const uint32_t v = mss_map_value(q[m.what]);
#pragma unroll
    for (int j = 0; j < kMssMapMaxThresholds; j++) cnt[j] += v > m.thr[j] ? 1u : 0u;
    return v;
}

// After the second barrier, in mss_lane's place: the lane's two outputs.  cnt[j] = how many of them lie in the valid region
// and exceed thr[j].  Block 1: they are stored, both in one 8-byte store where both are valid and the address allows it (vw
// may be odd: a row of the map need not start 8-byte aligned).  Cells: s_park[ly][lx / 2] = the larger of the valid ones, 0
// for none - a cell holds at least one valid position, so a 0 that stands for "outside" cannot become its maximum wrongly.
__device__ __forceinline__ void mss_map_lane(const mss_args &a, const mss_map_args &m, const double *s_col, uint32_t *s_park,
                                             uint32_t cnt[kMssMapMaxThresholds])
{
    const mss_where o = mss_block(a);
    const int lx = (threadIdx.x % (kMssTileW / 2)) * 2, ly = threadIdx.x / (kMssTileW / 2);
    double f0[kMssStreams], f1[kMssStreams];
    mss_rows(s_col, f0, f1);
#pragma unroll
    for (int j = 0; j < kMssMapMaxThresholds; j++) cnt[j] = 0;
    const uint32_t vw = a.w - kMssHalo, vh = a.h - kMssHalo, gx = o.x0 + lx, gy = o.y0 + ly;
    const bool in0 = gy < vh && gx < vw, in1 = gy < vh && gx + 1 < vw;
    uint32_t v0 = 0, v1 = 0;
    if (in0) v0 = mss_map_position(a, m, f0, cnt);
    if (in1) v1 = mss_map_position(a, m, f1, cnt);
    if (!m.map) return;
    if (m.lb) {
        s_park[ly * kMssPairsW + lx / 2] = v0 > v1 ? v0 : v1;
        return;
    }
    if (!in0) return;
    uint32_t *p = m.map + (((size_t)(blockIdx.y / 3u) * 3 + o.c) * vh + gy) * vw + gx;
    if (in1 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
        mss_u2 two;
        two.a = v0, two.b = v1;
        *reinterpret_cast<mss_u2 *>(p) = two;
    } else {
        p[0] = v0;
        if (in1) p[1] = v1;
    }
}

// The tile holds nx x ny cells, or is inside one (B = 32, 64: the tile's origin is a multiple of 32 and of 16)
__device__ __forceinline__ int mss_map_nx(const mss_map_args &m) { return m.lb < 5 ? kMssTileW >> m.lb : 1; }
__device__ __forceinline__ int mss_map_ny(const mss_map_args &m) { return m.lb < 4 ? kMssTileH >> m.lb : 1; }

// Behind a barrier after mss_map_lane (cells only): s_rows[r][i] = the maximum of row r of the tile over cell column i
__device__ __forceinline__ void mss_map_rows(const mss_map_args &m, const uint32_t *s_park, uint32_t *s_rows)
{
    const int nx = mss_map_nx(m), run = kMssPairsW / nx;  // parked values a cell's row
    if ((int)threadIdx.x >= nx * kMssTileH) return;
    const int r = threadIdx.x / nx, i = threadIdx.x % nx;
    uint32_t best = 0;
    for (int k = 0; k < run; k++) {
        const uint32_t v = s_park[r * kMssPairsW + i * run + k];
        best = v > best ? v : best;
    }
    s_rows[r * kMssPairsW + i] = best;
}

// Behind a barrier after mss_map_rows: the tile's cells.  B = 2 .. 16: the cell lies in this tile alone - the tile's origin
// is a multiple of B both ways - and is stored once.  B = 32, 64: the tile's one maximum goes into the cell it lies in with
// an atomic; the array starts at zero and only takes maxima, so a 0 has nothing to add.
__device__ __forceinline__ void mss_map_cells(const mss_args &a, const mss_map_args &m, const uint32_t *s_rows)
{
    const int nx = mss_map_nx(m), ny = mss_map_ny(m), run = kMssTileH / ny;
    if ((int)threadIdx.x >= nx * ny) return;
    const mss_where o = mss_block(a);
    const int j = threadIdx.x / nx, i = threadIdx.x % nx;
    const uint32_t cx = (o.x0 >> m.lb) + i, cy = (o.y0 >> m.lb) + j;
    if (cx >= m.cw || cy >= m.ch) return;
    uint32_t best = 0;
    for (int k = 0; k < run; k++) {
        const uint32_t v = s_rows[(j * run + k) * kMssPairsW + i];
        best = v > best ? v : best;
    }
    uint32_t *cell = m.map + (((size_t)(blockIdx.y / 3u) * 3 + o.c) * m.ch + cy) * m.cw + cx;
    if (m.lb < 5) *cell = best;
    else if (best) atomicMax(cell, best);
}

}  // namespace
