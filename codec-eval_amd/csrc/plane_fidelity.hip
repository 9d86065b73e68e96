// A decoder's Y'CbCr planes scored as planes (include/ce_metrics.h: ce_yuv_plane_fidelity): per pair and
// plane the exact squared error, and per level the two exact integers of SSIM / MS-SSIM as msssim.hip forms them, which the
// host finishes in f64.  Three kernels.  k_plane_sse, over (blocks, pairs x planes), streams the two sides' rows - pitched,
// possibly interleaved, possibly MSB-aligned - and adds one 64-bit integer per block with a vector atomic, as k_psnr_sse does.
// k_plane_level, over (tiles, pairs) for one plane and level, is k_msssim_level with another staging: level 0 reads the planes
// where they lie, through the plane table, the others the context's planar f32 pyramid.  k_plane_pool writes the next level of
// a run of images.  Integer sums do not depend on the order, so the scores do not depend on the grid.  The device code is
// plane_fidelity_kernel.h's, which a test also compiles for the host; here are the kernels' entry points, the reductions, the
// launches and the call itself.  The checks of the images and their upload are plane_images.h's, shared with plane_hvs.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ce_internal.h"

#include "plane_fidelity_kernel.h"

#include "plane_images.h"

namespace {

template <int BPS>
__global__ __launch_bounds__(kPfThreads) void k_plane_sse(const pf_sse_args a)
{
    __shared__ unsigned long long s_part[kPfWaves];
    unsigned long long sse = pf_sse_thread<BPS>(a);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sse += __shfl_down(sse, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sse;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < (int)kPfWaves; k++) t += s_part[k];
        const pf_where o = pf_sse_block(a);
        atomicAdd(a.out + (size_t)o.pair * kPfOut + o.plane, t);
    }
}

template <class SAMPLE>
__global__ __launch_bounds__(kMssThreads) void k_plane_level(const pf_level_args a)
{
    __shared__ float s_in[2 * kMssInLen];
    __shared__ __attribute__((aligned(16))) double s_col[kMssStreams * kMssColLen];
    __shared__ long long s_part[kMssThreads / 64][2];
    pf_stage<SAMPLE>(a, s_in);
    __syncthreads();
    mss_columns(s_in, s_col);
    __syncthreads();
    long long acc[2];
    mss_lane(a.m, s_col, acc);
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
        // [pair][3 + [plane][level][2]]; two's complement: the unsigned sum of signed addends is the signed sum
        atomicAdd(a.out + (size_t)(a.m.first + blockIdx.y) * kPfOut + 3 + ((size_t)a.plane * CE_MSSSIM_LEVELS + a.m.level) * 2 + threadIdx.x,
                  (unsigned long long)t);
    }
}

template <class SAMPLE>
__global__ __launch_bounds__(256) void k_plane_pool(const pf_pool_args a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)a.ow * a.oh) pf_pool_sample<SAMPLE>(a, i);
}

constexpr uint32_t kGridYMax = 65535;

// what the call has worked out about its images
struct pf_job {
    uint32_t n_refs = 0, n_pairs = 0, n_planes = 0, bps = 1, maxv = 255;
    uint32_t lw[3][CE_MSSSIM_LEVELS] = {}, lh[3][CE_MSSSIM_LEVELS] = {}, n_levels[3] = {};
    size_t pyr_off[3][CE_MSSSIM_LEVELS] = {};  // floats into the pyramid of plane p's level l = 1 .. n_levels[p] - 1
    const uint32_t *h_pair_ref = nullptr;      // host: pair -> reference
    const pf_plane *d_tab = nullptr;
    const uint32_t *d_pair_ref = nullptr;
    float *d_pyr = nullptr;
    unsigned long long *d_out = nullptr;
};

// kind: 0 u8 planes, 1 u16 planes, 2 the f32 pyramid; images [first, first + count)
int pool_run(ce_ctx *ctx, int kind, pf_pool_args a, uint32_t first, uint32_t count)
{
    const uint32_t bx = (uint32_t)(((size_t)a.ow * a.oh + 255) / 256);
    for (uint32_t done = 0; done < count; done += kGridYMax) {
        a.first = first + done;
        const dim3 grid(bx, std::min(count - done, kGridYMax));
        if (kind == 0) CE_LAUNCH(ctx, "plane_pool_u8", k_plane_pool<uint8_t>, grid, dim3(256), 0, a);
        else if (kind == 1) CE_LAUNCH(ctx, "plane_pool_u16", k_plane_pool<uint16_t>, grid, dim3(256), 0, a);
        else CE_LAUNCH(ctx, "plane_pool_f32", k_plane_pool<float>, grid, dim3(256), 0, a);
    }
    return CE_OK;
}

int launch(ce_ctx *ctx, const pf_job &j)
{
    CE_HIP(ctx, hipMemsetAsync(j.d_out, 0, sizeof(unsigned long long) * kPfOut * j.n_pairs, ctx->stream));
    // the squared error: one launch over (blocks of four rows, pairs x planes); a few pairs alone get up to a block per four
    // rows of luma (psnr.hip)
    {
        pf_sse_args a{};
        a.tab = j.d_tab, a.pair_ref = j.d_pair_ref, a.out = j.d_out, a.n_refs = j.n_refs, a.n_planes = j.n_planes, a.maxv = j.maxv;
        for (uint32_t p = 0; p < j.n_planes; p++) a.w[p] = j.lw[p][0], a.h[p] = j.lh[p][0];
        const uint32_t pairs_a_launch = kGridYMax / j.n_planes;
        for (uint32_t done = 0; done < j.n_pairs; done += pairs_a_launch) {
            const uint32_t count = std::min(j.n_pairs - done, pairs_a_launch);
            const uint32_t blocks = std::min((a.h[0] + kPfWaves - 1) / kPfWaves, std::max(64u, 4096u / count));
            a.first = done;
            if (j.bps == 1) CE_LAUNCH(ctx, "plane_sse_u8", k_plane_sse<1>, dim3(blocks, count * j.n_planes), dim3(kPfThreads), 0, a);
            else CE_LAUNCH(ctx, "plane_sse_u16", k_plane_sse<2>, dim3(blocks, count * j.n_planes), dim3(kPfThreads), 0, a);
        }
    }
    // the references the pairs name, as runs of consecutive images: each is pooled once
    std::vector<bool> named(j.n_refs, false);
    for (uint32_t i = 0; i < j.n_pairs; i++) named[j.h_pair_ref[i]] = true;
    std::vector<std::pair<uint32_t, uint32_t>> runs;  // first, count
    for (uint32_t r = 0; r < j.n_refs; r++)
        if (named[r]) {
            if (!runs.empty() && runs.back().first + runs.back().second == r) runs.back().second++;
            else runs.emplace_back(r, 1u);
        }
    const double maxv = (double)j.maxv;
    for (uint32_t p = 0; p < j.n_planes; p++)
        for (uint32_t l = 0; l < j.n_levels[p]; l++) {
            const uint32_t w = j.lw[p][l], h = j.lh[p][l];
            const int kind = l ? 2 : j.bps == 1 ? 0 : 1;
            pf_level_args g{};
            g.m.pair_ref = j.d_pair_ref, g.m.w = w, g.m.h = h, g.m.level = l;
            g.m.tiles_x = (w - kMssHalo + kMssTileW - 1) / kMssTileW;
            const uint32_t tiles_y = (h - kMssHalo + kMssTileH - 1) / kMssTileH;
            g.m.c1 = (0.01 * maxv) * (0.01 * maxv), g.m.c2 = (0.03 * maxv) * (0.03 * maxv);
            g.tab = j.d_tab, g.pyr = l ? j.d_pyr + j.pyr_off[p][l] : nullptr, g.out = j.d_out;
            g.n_refs = j.n_refs, g.plane = p, g.maxv = j.maxv;
            for (uint32_t done = 0; done < j.n_pairs; done += kGridYMax) {
                g.m.first = done;
                const dim3 grid(g.m.tiles_x * tiles_y, std::min(j.n_pairs - done, kGridYMax));
                if (kind == 0) CE_LAUNCH(ctx, "plane_level_u8", k_plane_level<uint8_t>, grid, dim3(kMssThreads), 0, g);
                else if (kind == 1) CE_LAUNCH(ctx, "plane_level_u16", k_plane_level<uint16_t>, grid, dim3(kMssThreads), 0, g);
                else CE_LAUNCH(ctx, "plane_level_f32", k_plane_level<float>, grid, dim3(kMssThreads), 0, g);
            }
            if (l + 1 == j.n_levels[p]) break;
            pf_pool_args q{};
            q.tab = j.d_tab, q.src = g.pyr, q.dst = j.d_pyr + j.pyr_off[p][l + 1], q.plane = p, q.maxv = j.maxv;
            q.w = w, q.h = h, q.ow = j.lw[p][l + 1], q.oh = j.lh[p][l + 1];
            for (const auto &run : runs)
                if (int rc = pool_run(ctx, kind, q, run.first, run.second)) return rc;
            if (int rc = pool_run(ctx, kind, q, j.n_refs, j.n_pairs)) return rc;  // the tests: one launch
        }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

double psnr_of(uint64_t sse, uint64_t n, double maxv)
{
    // ce_api.cpp: psnr_from_sse, on a plane's own count
    const double mse = (double)sse / (double)n;
    if (mse == 0.0) return INFINITY;
    return 10.0 * std::log10(maxv * maxv / mse);
}

}  // namespace

int ce_yuv_plane_fidelity(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs, const ce_yuv_image *tests,
                          uint32_t n_pairs, const uint32_t *pair_ref, uint32_t levels, ce_plane_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    const auto bad = [ctx](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, "plane fidelity: " + why); };
    if (int rc = pf_check_pairs(ctx, "plane fidelity", refs, n_refs, tests, n_pairs, pair_ref, out)) return rc;
    if (levels != 0 && levels != 1 && levels != CE_MSSSIM_LEVELS) return bad("levels must be 0 (PSNR), 1 (+ SSIM) or 5 (+ MS-SSIM), got " + std::to_string(levels));
    pf_images im;
    if (int rc = pf_check_images(ctx, "plane fidelity", width, height, refs, n_refs, tests, n_pairs, pair_ref, &im)) return rc;
    const size_t n_img = (size_t)n_refs + n_pairs;
    pf_job j;
    j.n_refs = n_refs, j.n_pairs = n_pairs, j.h_pair_ref = im.ref_of.data();
    j.n_planes = im.n_planes, j.bps = im.bps, j.maxv = im.maxv;
    if (levels) {  // luma must admit them
        uint32_t n = 0;
        if (int rc = ce_msssim_levels(width, height, levels, &n, j.lw[0], j.lh[0])) return ce_fail(ctx, rc, std::string("plane fidelity, luma: ") + ce_last_error(nullptr));
    }
    size_t pyr = 0;
    for (uint32_t p = 0; p < j.n_planes; p++) {
        const uint32_t pw = im.pw[p], ph = im.ph[p], m = std::min(pw, ph);
        j.n_levels[p] = levels == CE_MSSSIM_LEVELS && m > 160 ? CE_MSSSIM_LEVELS : levels >= 1 && m >= 11 ? 1 : 0;
        uint32_t w = pw, h = ph;
        for (uint32_t l = 0; l < std::max(j.n_levels[p], 1u); l++) {
            j.lw[p][l] = w, j.lh[p][l] = h;
            if (l) j.pyr_off[p][l] = pyr, pyr += n_img * w * h;
            w = (w + (w & 1u)) / 2, h = (h + (h & 1u)) / 2;
        }
    }
    // scratch: the pyramid and the results here; the planes and the tables in pf_upload (plane_images.h)
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->pf_pyr.reserve(ctx, pyr)) return rc;
    if (int rc = ctx->pf_out_h.reserve(ctx, (size_t)kPfOut * n_pairs)) return rc;
    if (int rc = ctx->pf_out_d.reserve(ctx, (size_t)kPfOut * n_pairs)) return rc;
    if (int rc = pf_upload(ctx, im, refs, tests)) return rc;
    j.d_tab = im.d_tab, j.d_pair_ref = im.d_pair_ref;
    j.d_pyr = ctx->pf_pyr, j.d_out = ctx->pf_out_d;
    if (int rc = launch(ctx, j)) return rc;
    CE_HIP(ctx, hipMemcpyAsync(ctx->pf_out_h.get(), ctx->pf_out_d.get(), sizeof(unsigned long long) * kPfOut * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the caller's planes are free again
    static const double wt[CE_MSSSIM_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    const double maxv = (double)j.maxv;
    for (uint32_t i = 0; i < n_pairs; i++) {
        const unsigned long long *r = ctx->pf_out_h.get() + (size_t)kPfOut * i;
        ce_plane_scores s{};
        s.n_planes = j.n_planes;
        uint64_t sse = 0, n = 0;
        for (uint32_t p = 0; p < 3; p++) {
            s.psnr[p] = s.ssim[p] = s.ms_ssim[p] = NAN;
            if (p >= j.n_planes) continue;
            s.sse[p] = r[p], s.n[p] = (uint64_t)j.lw[p][0] * j.lh[p][0];
            sse += s.sse[p], n += s.n[p];
            s.psnr[p] = psnr_of(s.sse[p], s.n[p], maxv);
            s.n_levels[p] = j.n_levels[p];
            double ms[CE_MSSSIM_LEVELS] = {}, mc[CE_MSSSIM_LEVELS] = {};
            for (uint32_t l = 0; l < j.n_levels[p]; l++) {
                const unsigned long long *q = r + 3 + ((size_t)p * CE_MSSSIM_LEVELS + l) * 2;
                s.ssim_q[p][l] = (int64_t)q[0], s.cs_q[p][l] = (int64_t)q[1];
                s.n_pos[p][l] = (uint64_t)(j.lw[p][l] - 10) * (j.lh[p][l] - 10);
                ms[l] = ((double)s.ssim_q[p][l] / 4294967296.0) / (double)s.n_pos[p][l];
                mc[l] = ((double)s.cs_q[p][l] / 4294967296.0) / (double)s.n_pos[p][l];
            }
            if (j.n_levels[p] >= 1) s.ssim[p] = ms[0];
            if (j.n_levels[p] == CE_MSSSIM_LEVELS) {
                double v = std::pow(std::max(mc[0], 0.0), wt[0]);
                for (int l = 1; l < 4; l++) v = v * std::pow(std::max(mc[l], 0.0), wt[l]);
                s.ms_ssim[p] = v * std::pow(std::max(ms[4], 0.0), wt[4]);
            }
        }
        s.psnr_weighted = ((6.0 * s.psnr[0] + s.psnr[1]) + s.psnr[2]) / 8.0;
        s.psnr_overall = psnr_of(sse, n, maxv);
        out[i] = s;
    }
    return CE_OK;
}
