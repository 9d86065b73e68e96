// The SSIM / MS-SSIM maps of RGB8 and equal-depth deep batches (include/ce_metrics.h: ce_batch_msssim_map):
// where a pair is bad at one level of section 27's pyramid.  k_msssim_level_map is k_msssim_level (msssim.hip) in the same frame -
// (tiles, pairs x channels), 256 threads, a 32 x 16 output tile, mss_stage and mss_columns unchanged, the score kernel's own
// per-position text - with other ends for a position's integer q: d = 2^32 - q saturated to 32 bits is stored (block 1), or
// maximised into its B x B cell - inside the block for B = 2 .. 16, whose cells never leave a tile, one plain store a cell; with
// one atomic per block for B = 32 and 64, whose cells span tiles - and compared with up to eight thresholds, the counts reduced
// like the scores: across the wave by shuffles, across the block in LDS, one u64 atomic per block and threshold in use.
// Maxima, integer sums and plain stores: nothing depends on the grid or on the order.  The device code is
// msssim_map_kernel.h's, which a test also compiles for the host; here are the kernel's entry point, the reduction of the
// counts and the launch.
#include "ce_internal.h"

#include "msssim_map_kernel.h"

namespace {

template <class SAMPLE>
__global__ __launch_bounds__(kMssThreads) void k_msssim_level_map(const mss_args a, const mss_map_args m, uint32_t n_thresholds,
                                                                  unsigned long long *__restrict__ over)
{
    __shared__ float s_in[2 * kMssInLen];
    __shared__ __attribute__((aligned(16))) double s_col[kMssStreams * kMssColLen];
    __shared__ uint32_t s_park[kMssParkLen], s_rows[kMssParkLen];
    __shared__ unsigned long long s_part[kMssThreads / 64][kMssMapMaxThresholds];
    mss_stage<SAMPLE>(a, s_in);
    __syncthreads();
    mss_columns(s_in, s_col);
    __syncthreads();
    uint32_t cnt[kMssMapMaxThresholds];
    mss_map_lane(a, m, s_col, s_park, cnt);
    if (m.map && m.lb) {  // the same for every lane of the launch
        __syncthreads();
        mss_map_rows(m, s_park, s_rows);
        __syncthreads();
        mss_map_cells(a, m, s_rows);
    }
    if (!over) return;  // the same for every lane of the launch
#pragma unroll
    for (int j = 0; j < kMssMapMaxThresholds; j++) {
        unsigned long long c = cnt[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][j] = c;
    }
    __syncthreads();
    if (threadIdx.x < n_thresholds) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < (int)kMssThreads / 64; w++) t += s_part[w][threadIdx.x];
        if (t) atomicAdd(over + (size_t)blockIdx.y * kMssMapMaxThresholds + threadIdx.x, t);  // [pair][channel][8]
    }
}

constexpr uint32_t kGridYMax = 65535;

}  // namespace

int ce_launch_msssim_map(ce_batch *b, uint32_t first, uint32_t count, uint32_t level, const uint32_t *lw, const uint32_t *lh, float *d_pyr,
                         uint32_t what, uint32_t block, uint32_t *d_map, const uint32_t *thresholds, uint32_t n_thresholds,
                         unsigned long long *d_over)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    if (int rc = ce_msssim_pool(b, first, count, 0, level, lw, lh, d_pyr)) return rc;
    const uint32_t depth = b->depth[0] ? b->depth[0] : 8;
    const double maxv = (double)((1u << depth) - 1u);
    const ce_msssim_planes p = ce_msssim_level_planes(b, level, lw, lh, d_pyr);
    mss_args g{};
    g.refs = p.refs, g.tests = p.tests, g.ref_slot = g.test_slot = p.slot, g.chan = p.chan, g.px = p.px;
    g.pair_ref = b->d_pair_ref, g.w = lw[level], g.h = lh[level], g.level = level;
    const uint32_t vw = g.w - kMssHalo, vh = g.h - kMssHalo;
    g.tiles_x = (vw + kMssTileW - 1) / kMssTileW;
    const uint32_t tiles_y = (vh + kMssTileH - 1) / kMssTileH;
    g.c1 = (0.01 * maxv) * (0.01 * maxv), g.c2 = (0.03 * maxv) * (0.03 * maxv);
    mss_map_args m{};
    m.what = what;
    while ((1u << m.lb) < block) m.lb++;
    m.cw = (vw + block - 1) >> m.lb, m.ch = (vh + block - 1) >> m.lb;
    const size_t pair_len = (size_t)3 * m.cw * m.ch;
    for (uint32_t j = 0; j < (uint32_t)kMssMapMaxThresholds; j++) m.thr[j] = j < n_thresholds ? thresholds[j] : 0xffffffffu;
    if (d_map && m.lb >= 5) CE_HIP(ctx, hipMemsetAsync(d_map, 0, sizeof(uint32_t) * pair_len * count, stream));
    if (d_over) CE_HIP(ctx, hipMemsetAsync(d_over, 0, sizeof(unsigned long long) * 3 * kMssMapMaxThresholds * count, stream));
    const uint32_t pairs_a_launch = kGridYMax / 3;
    for (uint32_t done = 0; done < count; done += pairs_a_launch) {
        g.first = first + done;
        m.map = d_map ? d_map + pair_len * done : nullptr;
        unsigned long long *over = d_over ? d_over + (size_t)3 * kMssMapMaxThresholds * done : nullptr;
        const dim3 grid(g.tiles_x * tiles_y, 3 * std::min(count - done, pairs_a_launch));
        if (p.kind == 0)
            CE_LAUNCH(ctx, "msssim_level_map_u8", k_msssim_level_map<uint8_t>, grid, dim3(kMssThreads), 0, g, m, n_thresholds, over);
        else if (p.kind == 1)
            CE_LAUNCH(ctx, "msssim_level_map_u16", k_msssim_level_map<uint16_t>, grid, dim3(kMssThreads), 0, g, m, n_thresholds, over);
        else
            CE_LAUNCH(ctx, "msssim_level_map_f32", k_msssim_level_map<float>, grid, dim3(kMssThreads), 0, g, m, n_thresholds, over);
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
