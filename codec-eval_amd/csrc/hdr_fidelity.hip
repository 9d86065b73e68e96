// HDR fidelity of a linear batch (include/ce_metrics.h: ce_batch_hdr_fidelity): PSNR in the PQ domain and
// the Delta E ITP of Rec. ITU-R BT.2124, as three exact integers per pair - the sum of squared PQ code differences, and the sum
// and the maximum of the per-pixel Delta E in units of 2^-20 - which the host finishes in f64.  One launch over
// (blocks, pairs) - one per 65535 pairs, which is what a grid's y holds - in psnr.hip's frame: the two f32 slabs through pair_ref, three u64 accumulators a lane, a reduction across
// the wave and the block, and one integer atomic per block and value.  Integer sums and maxima do not depend on the order, so
// the scores do not depend on the grid.
//
// 24 bytes in per pixel pair and twelve searches of the host-built threshold table (ce_tables.cpp: ce_build_pq_code_thresholds):
// a block keeps the table's coarse level in LDS - the whole table at depths 10 and 12 (4 and 16 KB), every 16th threshold at
// depth 16 (16 KB) - and finishes a depth-16 search in one 64-byte line of the global table.  No scratch.  The device code is
// hdr_fidelity_kernel.h's, which a test also compiles for the host; here are the kernel's entry point, its reduction and the
// launch.  The Delta E ITP maps (ce_batch_delta_e_itp_map) are a second kernel in the same frame, further
// down: the same per-pixel text with other ends, device code in hdr_fidelity_map_kernel.h.
#include "ce_internal.h"

#include "hdr_fidelity_map_kernel.h"

namespace {

template <int DEPTH>
__global__ __launch_bounds__(kHdrfThreads) void k_hdr_fidelity(const hdrf_args a, unsigned long long *__restrict__ out)
{
    __shared__ float s_tab[hdrf_coarse_len(DEPTH)];
    __shared__ unsigned long long s_part[kHdrfThreads / 64][3];
    hdrf_stage<DEPTH>(a, s_tab);
    __syncthreads();
    unsigned long long acc[3];
    hdrf_lane<DEPTH>(a, s_tab, acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc[0] += __shfl_down(acc[0], off, 64);
        acc[1] += __shfl_down(acc[1], off, 64);
        const unsigned long long m = __shfl_down(acc[2], off, 64);
        acc[2] = m > acc[2] ? m : acc[2];
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) s_part[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[3] = {0, 0, 0};
#pragma unroll
        for (int w = 0; w < (int)kHdrfThreads / 64; w++) {
            t[0] += s_part[w][0], t[1] += s_part[w][1];
            t[2] = s_part[w][2] > t[2] ? s_part[w][2] : t[2];
        }
        unsigned long long *o = out + (size_t)hdrf_pair(a) * 3;
        atomicAdd(o, t[0]);
        atomicAdd(o + 1, t[1]);
        atomicMax(o + 2, t[2]);
    }
}

// The Delta E ITP map of a pair (include/ce_metrics.h: ce_batch_delta_e_itp_map) in k_hdr_fidelity's
// frame: every pixel's k, saturated to 32 bits, stored (four to a 16-byte store on the wide path), or maximised into its
// B x B cell, or neither; and per lane how many exceed each of up to eight thresholds, reduced like the scores - across the
// wave by shuffles, across the block in LDS, one u64 atomic per block and threshold.  over == nullptr: no counts.
template <int DEPTH>
__global__ __launch_bounds__(kHdrfThreads) void k_delta_e_itp_map(const hdrf_args a, const hdrf_map_args m, uint32_t n_thresholds,
                                                                  unsigned long long *__restrict__ over)
{
    __shared__ float s_tab[hdrf_coarse_len(DEPTH)];
    __shared__ unsigned long long s_part[kHdrfThreads / 64][kItpMaxThresholds];
    hdrf_stage<DEPTH>(a, s_tab);
    __syncthreads();
    uint32_t cnt[kItpMaxThresholds];
    hdrf_map_lane<DEPTH>(a, m, s_tab, cnt);
    if (!over) return;  // the same for every lane of the launch
#pragma unroll
    for (int j = 0; j < kItpMaxThresholds; j++) {
        unsigned long long c = cnt[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][j] = c;
    }
    __syncthreads();
    if (threadIdx.x < n_thresholds) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < (int)kHdrfThreads / 64; w++) t += s_part[w][threadIdx.x];
        if (t) atomicAdd(over + (size_t)hdrf_pair(a) * kItpMaxThresholds + threadIdx.x, t);
    }
}

// what both launches hand their kernel: pairs [first, ...) of the batch at `depth`; a launch then takes a range of those
// (hdrf_args::first), at most ce_grid_yz_max to a grid's y
hdrf_args hdrf_fill(const ce_batch *b, uint32_t first, uint32_t depth, const float *d_table, const float *d_coarse, const float a[9],
                    const float lms[9])
{
    hdrf_args g{};
    g.n_pixels = (size_t)b->w * b->h;
    g.refs = reinterpret_cast<const float *>(b->d_refs.get());
    g.tests = reinterpret_cast<const float *>(b->d_tests.get()) + (size_t)first * g.n_pixels * 3;
    g.pair_ref = b->d_pair_ref + first, g.table = d_table, g.coarse = d_coarse;
    for (int i = 0; i < 9; i++) g.a[i] = a[i], g.b[i] = lms[i];
    g.denom = 4096.0 * (double)((1u << depth) - 1u);
    return g;
}

}  // namespace

int ce_launch_hdr_fidelity(ce_batch *b, uint32_t n_pairs, uint32_t depth, const float *d_table, const float *d_coarse, const float a[9],
                           const float lms[9], unsigned long long *d_out)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    CE_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * 3 * n_pairs, stream));
    hdrf_args g = hdrf_fill(b, 0, depth, d_table, d_coarse, a, lms);
    const uint32_t blocks = hdrf_blocks(g.n_pixels, n_pairs);
    for (g.first = 0; g.first < n_pairs; g.first += ce_grid_yz_max) {
        const dim3 grid(blocks, std::min(n_pairs - g.first, ce_grid_yz_max));
        switch (depth) {
            case 10: CE_LAUNCH(ctx, "hdr_fidelity_10", k_hdr_fidelity<10>, grid, dim3(kHdrfThreads), 0, g, d_out); break;
            case 12: CE_LAUNCH(ctx, "hdr_fidelity_12", k_hdr_fidelity<12>, grid, dim3(kHdrfThreads), 0, g, d_out); break;
            case 16: CE_LAUNCH(ctx, "hdr_fidelity_16", k_hdr_fidelity<16>, grid, dim3(kHdrfThreads), 0, g, d_out); break;
            default: ctx->err = "HDR fidelity: depth must be 10, 12 or 16"; return CE_ERR_INVALID_ARG;
        }
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

int ce_launch_delta_e_itp_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t depth, const float *d_table, const float *d_coarse,
                              const float a[9], const float lms[9], uint32_t block, uint32_t *d_map, const uint32_t *thresholds,
                              uint32_t n_thresholds, unsigned long long *d_over)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    hdrf_args g = hdrf_fill(b, first, depth, d_table, d_coarse, a, lms);
    hdrf_map_args m{};
    m.map = d_map, m.w = b->w;
    while ((1u << m.lb) < block) m.lb++;
    m.cw = (b->w + block - 1) >> m.lb;
    m.pair_len = (size_t)m.cw * ((b->h + block - 1) >> m.lb);
    for (uint32_t j = 0; j < (uint32_t)kItpMaxThresholds; j++) m.thr[j] = j < n_thresholds ? thresholds[j] : 0xffffffffu;
    if (d_map && m.lb) CE_HIP(ctx, hipMemsetAsync(d_map, 0, sizeof(uint32_t) * m.pair_len * count, stream));
    if (d_over) CE_HIP(ctx, hipMemsetAsync(d_over, 0, sizeof(unsigned long long) * kItpMaxThresholds * count, stream));
    const uint32_t blocks = hdrf_blocks(g.n_pixels, count);
    for (g.first = 0; g.first < count; g.first += ce_grid_yz_max) {
        const dim3 grid(blocks, std::min(count - g.first, ce_grid_yz_max));
        switch (depth) {
            case 10: CE_LAUNCH(ctx, "delta_e_itp_map_10", k_delta_e_itp_map<10>, grid, dim3(kHdrfThreads), 0, g, m, n_thresholds, d_over); break;
            case 12: CE_LAUNCH(ctx, "delta_e_itp_map_12", k_delta_e_itp_map<12>, grid, dim3(kHdrfThreads), 0, g, m, n_thresholds, d_over); break;
            case 16: CE_LAUNCH(ctx, "delta_e_itp_map_16", k_delta_e_itp_map<16>, grid, dim3(kHdrfThreads), 0, g, m, n_thresholds, d_over); break;
            default: ctx->err = "Delta E ITP map: depth must be 10, 12 or 16"; return CE_ERR_INVALID_ARG;
        }
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
