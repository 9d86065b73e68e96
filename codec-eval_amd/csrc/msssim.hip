// SSIM and MS-SSIM of RGB8 and equal-depth deep batches (include/ce_metrics.h: ce_batch_msssim): per pair,
// level and channel two exact integers - the sums of the per-position SSIM and contrast-structure values in units of 2^-32 -
// which the host finishes in f64.  Two kernels.  k_msssim_level, over (tiles, pairs x channels), is a level fused: a block
// stages its 32 x 16 outputs' 42 x 26 samples of both planes in LDS (level 0 straight from the u8 / u16 slabs), filters the five
// streams x, y, x*x, y*y, x*y down the columns into LDS, then along the rows in registers, forms s and cs, quantises them, reduces
// across the wave and the block and adds one 64-bit integer per block and value with a vector atomic, as k_hdr_fidelity does.
// k_msssim_pool writes the next level of a run of slots into the batch's f32 pyramid.  Integer sums do not depend on the
// order, so the scores do not depend on the grid.  The device code is msssim_kernel.h's, which a test also compiles for the
// host; here are the kernels' entry points, the reduction and the launches.
#include "ce_internal.h"

#include "msssim_kernel.h"

namespace {

template <class SAMPLE>
__global__ __launch_bounds__(kMssThreads) void k_msssim_level(const mss_args a, unsigned long long *__restrict__ out)
{
    __shared__ float s_in[2 * kMssInLen];
    __shared__ __attribute__((aligned(16))) double s_col[kMssStreams * kMssColLen];
    __shared__ long long s_part[kMssThreads / 64][2];
    mss_stage<SAMPLE>(a, s_in);
    __syncthreads();
    mss_columns(s_in, s_col);
    __syncthreads();
    long long acc[2];
    mss_lane(a, s_col, acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc[0] += __shfl_down(acc[0], off, 64);
        acc[1] += __shfl_down(acc[1], off, 64);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][0] = acc[0], s_part[threadIdx.x >> 6][1] = acc[1];
    __syncthreads();
    if (threadIdx.x < 2) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < (int)kMssThreads / 64; w++) t += s_part[w][threadIdx.x];
        const mss_where o = mss_block(a);
        // [pair][level][channel][2]; two's complement: the unsigned sum of signed addends is the signed sum
        atomicAdd(out + (((size_t)o.pair * CE_MSSSIM_LEVELS + a.level) * 3 + o.c) * 2 + threadIdx.x, (unsigned long long)t);
    }
}

template <class SAMPLE>
__global__ __launch_bounds__(256) void k_msssim_pool(const mss_pool_args a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)3 * a.ow * a.oh) mss_pool_sample<SAMPLE>(a, i);
}

constexpr uint32_t kGridYMax = 65535;

// kind: 0 u8 slabs, 1 u16 slabs, 2 the f32 pyramid
int pool_run(ce_ctx *ctx, int kind, mss_pool_args a, uint32_t first, uint32_t count)
{
    const uint32_t bx = (uint32_t)(((size_t)3 * a.ow * a.oh + 255) / 256);
    for (uint32_t done = 0; done < count; done += kGridYMax) {
        a.first = first + done;
        const dim3 grid(bx, std::min(count - done, kGridYMax));
        if (kind == 0) CE_LAUNCH(ctx, "msssim_pool_u8", k_msssim_pool<uint8_t>, grid, dim3(256), 0, a);
        else if (kind == 1) CE_LAUNCH(ctx, "msssim_pool_u16", k_msssim_pool<uint16_t>, grid, dim3(256), 0, a);
        else CE_LAUNCH(ctx, "msssim_pool_f32", k_msssim_pool<float>, grid, dim3(256), 0, a);
    }
    return CE_OK;
}

// the pyramid: level l = 1 .. 4 at this many floats, [slots][3][lh[l]][lw[l]]
size_t pyr_off(const ce_batch *b, uint32_t l, const uint32_t *lw, const uint32_t *lh)
{
    const size_t slots = (size_t)b->max_refs + b->max_pairs;
    size_t off = 0;
    for (uint32_t k = 1; k < l; k++) off += slots * 3 * lw[k] * lh[k];
    return off;
}

}  // namespace

ce_msssim_planes ce_msssim_level_planes(const ce_batch *b, uint32_t l, const uint32_t *lw, const uint32_t *lh, float *d_pyr)
{
    const size_t plane = (size_t)lw[l] * lh[l], off = pyr_off(b, l, lw, lh);
    ce_msssim_planes p{};
    p.refs = l ? static_cast<const void *>(d_pyr + off) : static_cast<const void *>(b->d_refs.get());
    p.tests = l ? static_cast<const void *>(d_pyr + off + (size_t)b->max_refs * 3 * plane) : static_cast<const void *>(b->d_tests.get());
    p.slot = 3 * plane, p.chan = l ? plane : 1, p.px = l ? 1 : 3;
    p.kind = l ? 2 : (b->depth[0] ? 1 : 0);
    return p;
}

int ce_msssim_pool(ce_batch *b, uint32_t first, uint32_t count, uint32_t from, uint32_t last, const uint32_t *lw, const uint32_t *lh,
                   float *d_pyr)
{
    if (from >= last) return CE_OK;
    ce_ctx *ctx = b->ctx;
    // the reference slots the pairs name, as runs of consecutive slots: each is pooled once
    std::vector<bool> named(b->max_refs, false);
    for (uint32_t i = 0; i < count; i++) named[b->h_pair_ref[first + i]] = true;
    std::vector<std::pair<uint32_t, uint32_t>> runs;  // first, count
    for (uint32_t r = 0; r < b->max_refs; r++)
        if (named[r]) {
            if (!runs.empty() && runs.back().first + runs.back().second == r) runs.back().second++;
            else runs.emplace_back(r, 1u);
        }
    for (uint32_t l = from; l < last; l++) {
        const ce_msssim_planes src = ce_msssim_level_planes(b, l, lw, lh, d_pyr);
        float *dst = d_pyr + pyr_off(b, l + 1, lw, lh);
        mss_pool_args p{};
        p.src_slot = src.slot, p.chan = src.chan, p.px = src.px, p.w = lw[l], p.h = lh[l], p.ow = lw[l + 1], p.oh = lh[l + 1];
        p.dst_slot = (size_t)3 * p.ow * p.oh;
        p.src = src.refs, p.dst = dst;
        for (const auto &run : runs)
            if (int rc = pool_run(ctx, src.kind, p, run.first, run.second)) return rc;
        p.src = src.tests, p.dst = dst + (size_t)b->max_refs * p.dst_slot;
        if (int rc = pool_run(ctx, src.kind, p, first, count)) return rc;
    }
    return CE_OK;
}

int ce_launch_msssim(ce_batch *b, uint32_t n_pairs, uint32_t levels, const uint32_t *lw, const uint32_t *lh, float *d_pyr,
                     unsigned long long *d_out)
{
    ce_ctx *ctx = b->ctx;
    hipStream_t stream = CE_STREAM(ctx);
    CE_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * CE_MSSSIM_LEVELS * 6 * n_pairs, stream));
    const uint32_t depth = b->depth[0] ? b->depth[0] : 8;
    const double maxv = (double)((1u << depth) - 1u);
    for (uint32_t l = 0; l < levels; l++) {
        const ce_msssim_planes p = ce_msssim_level_planes(b, l, lw, lh, d_pyr);
        mss_args g{};
        g.refs = p.refs, g.tests = p.tests, g.ref_slot = g.test_slot = p.slot, g.chan = p.chan, g.px = p.px;
        g.pair_ref = b->d_pair_ref, g.w = lw[l], g.h = lh[l], g.level = l;
        g.tiles_x = (lw[l] - kMssHalo + kMssTileW - 1) / kMssTileW;
        const uint32_t tiles_y = (lh[l] - kMssHalo + kMssTileH - 1) / kMssTileH;
        g.c1 = (0.01 * maxv) * (0.01 * maxv), g.c2 = (0.03 * maxv) * (0.03 * maxv);
        const uint32_t pairs_a_launch = kGridYMax / 3;
        for (uint32_t done = 0; done < n_pairs; done += pairs_a_launch) {
            g.first = done;
            const dim3 grid(g.tiles_x * tiles_y, 3 * std::min(n_pairs - done, pairs_a_launch));
            if (p.kind == 0) CE_LAUNCH(ctx, "msssim_level_u8", k_msssim_level<uint8_t>, grid, dim3(kMssThreads), 0, g, d_out);
            else if (p.kind == 1) CE_LAUNCH(ctx, "msssim_level_u16", k_msssim_level<uint16_t>, grid, dim3(kMssThreads), 0, g, d_out);
            else CE_LAUNCH(ctx, "msssim_level_f32", k_msssim_level<float>, grid, dim3(kMssThreads), 0, g, d_out);
        }
        if (l + 1 == levels) break;
        if (int rc = ce_msssim_pool(b, 0, n_pairs, l, l + 1, lw, lh, d_pyr)) return rc;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

// the window as the kernel has it
extern "C" int ce_msssim_window(double out[11])
{
    if (!out) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_msssim_window: null pointer");
    for (int i = 0; i < kMssTaps; i++) out[i] = mss_g(i);
    return CE_OK;
}
