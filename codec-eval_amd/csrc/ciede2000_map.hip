// The CIEDE2000 maps of an RGB8 or deep batch (include/ce_metrics.h: ce_batch_ciede2000_map): per pixel
// of a pair one of four values in units of 2^-20 - q itself, the very integer k_ciede2000 sums, or the magnitude of its
// lightness, chroma or hue term - stored (four to a 16-byte store on the wide path), or maximised into its B x B cell, or
// neither; and per lane how many exceed each of up to eight thresholds, reduced like the scores - across the wave by shuffles,
// across the block in LDS, one u64 vector atomic per block and threshold.  One launch over (blocks, pairs) - one per 65535
// pairs - in k_ciede2000's frame and geometry (cie_blocks).  The arithmetic is the score kernel's, about 1350 f64 instructions a
// pixel against 4 bytes out: bound by the vector f64 rate.  No scratch.  The device code is ciede2000_map_kernel.h's, which a
// test also compiles for the host; here are the kernel's entry point, its reduction and the launch.
#include "ce_internal.h"

#include "ciede2000_map_kernel.h"

namespace {

// over == nullptr: no counts
template <bool DEEP>
__global__ __launch_bounds__(kCieThreads) void k_ciede2000_map(const cie_args a, const cie_map_args m, uint32_t n_thresholds,
                                                                unsigned long long *__restrict__ over)
{
    extern __shared__ float s_tab[];
    __shared__ unsigned long long s_part[kCieThreads / 64][kCieMaxThresholds];
    cie_stage(a, s_tab);
    __syncthreads();
    uint32_t cnt[kCieMaxThresholds];
    cie_map_lane<DEEP>(a, m, s_tab, cnt);
    if (!over) return;  // the same for every lane of the launch
#pragma unroll
    for (int j = 0; j < kCieMaxThresholds; j++) {
        unsigned long long c = cnt[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][j] = c;
    }
    __syncthreads();
    if (threadIdx.x < n_thresholds) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < (int)kCieThreads / 64; w++) t += s_part[w][threadIdx.x];
        if (t) atomicAdd(over + (size_t)cie_pair(a) * kCieMaxThresholds + threadIdx.x, t);
    }
}

}  // namespace

int ce_launch_ciede2000_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t what, const float *d_table_ref, const float *d_table_test,
                            uint32_t block, uint32_t *d_map, const uint32_t *thresholds, uint32_t n_thresholds, unsigned long long *d_over)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    const bool deep = b->depth[0] != 0;
    cie_args g{};
    g.n_pixels = (size_t)b->w * b->h;
    // pairs [first, ...) of the batch; a launch then takes a range of those (cie_args::first), at most ce_grid_yz_max to a grid's y
    g.refs = b->d_refs.get();
    g.tests = static_cast<const uint8_t *>(b->d_tests.get()) + (size_t)first * g.n_pixels * 3 * (deep ? 2 : 1);
    g.pair_ref = b->d_pair_ref + first;
    g.table[0] = d_table_ref, g.table[1] = d_table_test;
    g.depth[0] = deep ? b->depth[0] : 8, g.depth[1] = deep ? b->depth[1] : 8;
    for (uint32_t j = 0; j < (uint32_t)kCieMaxThresholds; j++) g.thr[j] = j < n_thresholds ? thresholds[j] : 0xffffffffu;
    cie_map_args m{};
    m.map = d_map, m.what = what, m.w = b->w;
    while ((1u << m.lb) < block) m.lb++;
    m.cw = (b->w + block - 1) >> m.lb;
    m.pair_len = (size_t)m.cw * ((b->h + block - 1) >> m.lb);
    if (d_map && m.lb) CE_HIP(ctx, hipMemsetAsync(d_map, 0, sizeof(uint32_t) * m.pair_len * count, stream));
    if (d_over) CE_HIP(ctx, hipMemsetAsync(d_over, 0, sizeof(unsigned long long) * kCieMaxThresholds * count, stream));
    const uint32_t blocks = cie_blocks(g.n_pixels, count, deep);
    const size_t lds = sizeof(float) * cie_lds_floats(g.depth[0], g.depth[1]);
    for (g.first = 0; g.first < count; g.first += ce_grid_yz_max) {
        const dim3 grid(blocks, std::min(count - g.first, ce_grid_yz_max));
        if (deep) CE_LAUNCH(ctx, "ciede2000_map_u16", k_ciede2000_map<true>, grid, dim3(kCieThreads), lds, g, m, n_thresholds, d_over);
        else CE_LAUNCH(ctx, "ciede2000_map_u8", k_ciede2000_map<false>, grid, dim3(kCieThreads), lds, g, m, n_thresholds, d_over);
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
