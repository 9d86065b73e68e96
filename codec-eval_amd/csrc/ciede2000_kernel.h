// The device code of the CIEDE2000 scores (ciede2000.hip; include/ce_metrics.h: ce_batch_ciede2000), kept
// like hdr_fidelity_kernel.h free of anything but the HIP keywords, uint4 and blockIdx / threadIdx / gridDim, so that
// tests/cpp/ciede2000_kernel_host.cpp can compile the same text for the host and run it under the host sanitizers.
// k_ciede2000 is split at its barrier for that: cie_stage fills the LDS, cie_lane reads it and returns the lane's integers;
// the reduction across lanes stays in ciede2000.hip.  The pixel is ciede2000_pixel.h's.
//
// DEEP says what the slabs hold - packed u8 RGB (an RGB8 batch, read through the 8-bit table) or packed u16 RGB at the two
// sides' own depths - and the depths are run-time arguments: a table of up to 12 bits (16 KB) is staged in LDS, once where the
// two sides share a depth, and the 16-bit one (256 KB) is gathered from global memory.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ciede2000_pixel.h"

namespace {

constexpr uint32_t kCieThreads = 256;
constexpr int kCieMaxThresholds = 8;   // CE_CIEDE2000_MAX_THRESHOLDS
constexpr uint32_t kCieLdsDepth = 12;  // the deepest table a block keeps in LDS
constexpr int kCieOut = 2 + kCieMaxThresholds;  // u64 per pair on the device: sum_q20, max_q20, n_above[8]

struct cie_args {
    const void *refs, *tests;   // the batch's slabs: n_pixels * 3 samples per slot, u8 or u16
    const uint32_t *pair_ref;   // pair -> reference slot
    const float *table[2];      // ce_srgb_table(depth, 0) of the reference / the test side: 2^depth floats
    uint32_t depth[2];          // 8, 10, 12 or 16 (8 / 8 for an RGB8 batch)
    size_t n_pixels;
    uint32_t thr[kCieMaxThresholds];  // q > thr[j] is counted; 2^32 - 1 past the caller's thresholds
    uint32_t first;             // the launch's pairs are [first, first + gridDim.y)
};

// the pair of this block
__device__ __forceinline__ uint32_t cie_pair(const cie_args &a) { return a.first + blockIdx.y; }

// what a lane carries: the sum and the maximum of its pixels' q and how many exceed each threshold
struct cie_acc {
    unsigned long long sum;
    uint32_t max, cnt[kCieMaxThresholds];
};

// the floats of LDS a block stages: each side's table where it is at most 12 bits deep, one copy where the depths agree
constexpr uint32_t cie_lds_side(uint32_t depth) { return depth <= kCieLdsDepth ? 1u << depth : 0u; }
inline uint32_t cie_lds_floats(uint32_t depth_ref, uint32_t depth_test)
{
    return cie_lds_side(depth_ref) + (depth_test == depth_ref ? 0u : cie_lds_side(depth_test));
}

// pixels of a lane's unit of work: on the wide path - an image whose byte size is a multiple of 16, so that every image of a
// slab starts 16-byte aligned - three 16-byte loads a side, which hold 16 u8 pixels or 8 u16 pixels; one pixel otherwise
constexpr uint32_t cie_unit(bool deep) { return deep ? 8u : 16u; }
constexpr bool cie_wide(size_t n_pixels, bool deep) { return n_pixels % cie_unit(deep) == 0; }

// The blocks a pair gets in a launch of n_pairs, as hdrf_blocks: a block has up to 32 KB of tables to stage and a pixel is
// some thousand instructions, so at most 64 blocks a pair, or what keeps a launch of few pairs near 1024 blocks.
inline uint32_t cie_blocks(size_t n_pixels, uint32_t n_pairs, bool deep)
{
    const size_t work = cie_wide(n_pixels, deep) ? n_pixels / cie_unit(deep) : n_pixels;
    const size_t want = (work + kCieThreads - 1) / kCieThreads, cap = 1024 / n_pairs > 64 ? 1024 / n_pairs : 64;
    return (uint32_t)(want > cap ? cap : want ? want : 1);
}

// one side's table as a lane reads it: from LDS, or (lds == nullptr) from global memory
struct cie_tab {
    const float *lds, *glob;
    uint32_t maxv;
};
__device__ __forceinline__ float cie_lookup(const cie_tab &t, uint32_t v)
{
    v = v < t.maxv ? v : t.maxv;
    if (t.lds) return t.lds[v];
    return t.glob[v];
}

// Before the barrier: the tables of at most 12 bits into s_tab, the reference side's first.
__device__ __forceinline__ void cie_stage(const cie_args &a, float *s_tab)
{
    const uint32_t n0 = cie_lds_side(a.depth[0]), n1 = a.depth[1] == a.depth[0] ? 0u : cie_lds_side(a.depth[1]);
    for (uint32_t i = threadIdx.x; i < n0; i += kCieThreads) s_tab[i] = a.table[0][i];
    for (uint32_t i = threadIdx.x; i < n1; i += kCieThreads) s_tab[n0 + i] = a.table[1][i];
}

// where cie_stage put them
__device__ __forceinline__ void cie_tabs(const cie_args &a, const float *s_tab, cie_tab &tr, cie_tab &tt)
{
    const uint32_t n0 = cie_lds_side(a.depth[0]);
    tr.lds = n0 ? s_tab : nullptr, tr.glob = a.table[0], tr.maxv = (1u << a.depth[0]) - 1u;
    tt.lds = a.depth[1] == a.depth[0] ? tr.lds : cie_lds_side(a.depth[1]) ? s_tab + n0 : nullptr;
    tt.glob = a.table[1], tt.maxv = (1u << a.depth[1]) - 1u;
}

// one pixel of a pair into the lane's integers.  Two equal code triples at one depth are two equal Lab values, whose q is 0:
// the sum, the maximum and every count stay as they are, so the arithmetic is skipped.
__device__ __forceinline__ void cie_pixel(const cie_args &a, const cie_tab &tr, const cie_tab &tt, const uint32_t r[3], const uint32_t t[3],
                                          cie_acc &acc)
{
    if (a.depth[0] == a.depth[1] && r[0] == t[0] && r[1] == t[1] && r[2] == t[2]) return;
    const float er[3] = {cie_lookup(tr, r[0]), cie_lookup(tr, r[1]), cie_lookup(tr, r[2])};
    const float et[3] = {cie_lookup(tt, t[0]), cie_lookup(tt, t[1]), cie_lookup(tt, t[2])};
    const uint32_t q = cie_pixel_q20(er, et);
    acc.sum += q;
    acc.max = q > acc.max ? q : acc.max;
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) acc.cnt[j] += q > a.thr[j] ? 1u : 0u;
}

// After the barrier: this lane's share of pair first + blockIdx.y, in k_hdr_fidelity's frame.  On the wide path a lane's unit is the
// twelve dwords of three 16-byte loads a side; its pixels are taken from the low end one at a time - the loop is not unrolled,
// the pixel being some thousand instructions - and the dwords are shifted down by a pixel (3 or 6 bytes) in between, so that
// no register is indexed by a variable.
template <bool DEEP>
__device__ __forceinline__ void cie_lane(const cie_args &a, const float *s_tab, cie_acc &acc)
{
    cie_tab tr, tt;
    cie_tabs(a, s_tab, tr, tt);
    const uint32_t p = cie_pair(a);
    const size_t img = a.n_pixels * 3 * (DEEP ? 2 : 1);  // bytes
    const uint8_t *ref = static_cast<const uint8_t *>(a.refs) + (size_t)a.pair_ref[p] * img;
    const uint8_t *test = static_cast<const uint8_t *>(a.tests) + (size_t)p * img;
    const size_t tid = (size_t)blockIdx.x * kCieThreads + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * kCieThreads;
    acc.sum = 0, acc.max = 0;
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) acc.cnt[j] = 0;
    if (cie_wide(a.n_pixels, DEEP)) {
        const uint4 *r4 = reinterpret_cast<const uint4 *>(ref);
        const uint4 *t4 = reinterpret_cast<const uint4 *>(test);
        for (size_t i = tid; i < a.n_pixels / cie_unit(DEEP); i += nthreads) {
            const uint4 r0 = r4[i * 3], r1 = r4[i * 3 + 1], r2 = r4[i * 3 + 2];
            const uint4 t0 = t4[i * 3], t1 = t4[i * 3 + 1], t2 = t4[i * 3 + 2];
            uint32_t rw[14] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, 0u, 0u};
            uint32_t tw[14] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, 0u, 0u};
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
                cie_pixel(a, tr, tt, r, t, acc);
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
            cie_pixel(a, tr, tt, r, t, acc);
        }
    }
}

}  // namespace
