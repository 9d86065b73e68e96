// CIEDE2000 of an RGB8 or deep batch (include/ce_metrics.h: ce_batch_ciede2000): per pair the sum and
// the maximum of the per-pixel colour difference in units of 2^-20 and how many pixels exceed each of up to eight thresholds -
// exact integers, which the host finishes in f64.  One launch over (blocks, pairs) - one per 65535 pairs - in k_hdr_fidelity's frame: the two slabs
// through pair_ref, a u64 sum, a maximum and eight counts a lane, a reduction across the wave by shuffles and across the block
// in LDS, and one integer vector atomic per block and value.  Integer sums, maxima and counts do not depend on the order, so
// the scores do not depend on the grid.
//
// 6 or 12 bytes in per pixel pair and about 700 f64 operations, 40 of them divisions and 9 square roots (ciede2000_pixel.h):
// the kernel is bound by the vector f64 rate, not by memory.  A block keeps the sRGB tables of up to 12 bits in dynamic LDS
// (1 to 32 KB) and gathers a 16-bit table from global memory.  No scratch.  The device code is ciede2000_kernel.h's, which a test also compiles for the host; here are
// the kernel's entry point, its reduction and the launch.
#include "ce_internal.h"

#include "ciede2000_kernel.h"

namespace {

template <bool DEEP>
__global__ __launch_bounds__(kCieThreads) void k_ciede2000(const cie_args a, unsigned long long *__restrict__ out)
{
    extern __shared__ float s_tab[];
    __shared__ unsigned long long s_part[kCieThreads / 64][kCieOut];
    cie_stage(a, s_tab);
    __syncthreads();
    cie_acc acc;
    cie_lane<DEEP>(a, s_tab, acc);
    unsigned long long v[kCieOut];
    v[0] = acc.sum, v[1] = acc.max;
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) v[2 + j] = acc.cnt[j];
#pragma unroll
    for (int j = 0; j < kCieOut; j++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(v[j], off, 64);
            v[j] = j == 1 ? (o > v[j] ? o : v[j]) : v[j] + o;
        }
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kCieOut) {
        const uint32_t j = threadIdx.x;
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < (int)kCieThreads / 64; w++) t = j == 1 ? (s_part[w][j] > t ? s_part[w][j] : t) : t + s_part[w][j];
        unsigned long long *o = out + (size_t)cie_pair(a) * kCieOut + j;
        if (t) {
            if (j == 1) atomicMax(o, t); else atomicAdd(o, t);
        }
    }
}

}  // namespace

int ce_launch_ciede2000(ce_batch *b, uint32_t n_pairs, const float *d_table_ref, const float *d_table_test, const uint32_t *thresholds,
                        uint32_t n_thresholds, unsigned long long *d_out)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    CE_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * kCieOut * n_pairs, stream));
    const bool deep = b->depth[0] != 0;
    cie_args g{};
    g.refs = b->d_refs.get(), g.tests = b->d_tests.get(), g.pair_ref = b->d_pair_ref;
    g.table[0] = d_table_ref, g.table[1] = d_table_test;
    g.depth[0] = deep ? b->depth[0] : 8, g.depth[1] = deep ? b->depth[1] : 8;
    g.n_pixels = (size_t)b->w * b->h;
    for (uint32_t j = 0; j < (uint32_t)kCieMaxThresholds; j++) g.thr[j] = j < n_thresholds ? thresholds[j] : 0xffffffffu;
    const uint32_t blocks = cie_blocks(g.n_pixels, n_pairs, deep);
    const size_t lds = sizeof(float) * cie_lds_floats(g.depth[0], g.depth[1]);
    // pairs [first, first + count) a launch: a grid's y holds at most ce_grid_yz_max pairs
    for (g.first = 0; g.first < n_pairs; g.first += ce_grid_yz_max) {
        const dim3 grid(blocks, std::min(n_pairs - g.first, ce_grid_yz_max));
        if (deep) CE_LAUNCH(ctx, "ciede2000_u16", k_ciede2000<true>, grid, dim3(kCieThreads), lds, g, d_out);
        else CE_LAUNCH(ctx, "ciede2000_u8", k_ciede2000<false>, grid, dim3(kCieThreads), lds, g, d_out);
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
