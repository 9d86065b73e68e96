// GMSD of a decoder's Y'CbCr planes (include/ce_metrics.h: ce_yuv_plane_gmsd): per pair and plane the
// exact sum of the quantised gradient magnitude similarities q, their exact second moment and the largest 2^32 - q, which the
// host finishes into the deviation (GMSD) and the mean (GMSM).  One kernel, k_plane_gmsd, over (tiles of 64 x 16 positions, pairs
// x planes) in one launch as k_plane_sse and k_plane_hvs share theirs among the planes: the 2 x 2 sums of both sides staged in
// LDS with a rim of one (plane_gmsd_kernel.h: gmsd_stage), one barrier, four positions a thread (gmsd_score), then the thread
// block's five integers reduced as k_plane_hvs reduces its two - shuffles, LDS across the waves - and handed over with vector
// atomics.  The second moment travels as sum qh qh, sum qh ql and sum ql ql with q = qh 2^16 + ql: each term is at most 2^32
// and a plane has under 2^32 positions, so no accumulator can wrap; the host combines them in 128 bits.  The planes are read
// where they lie through plane_fidelity_kernel.h's table; the checks and the upload are plane_images.h's, shared with the
// other plane calls.  The device code is plane_gmsd_kernel.h's, which a test also compiles for the host.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ce_internal.h"

#include "plane_gmsd_kernel.h"

#include "plane_images.h"

static_assert(sizeof(ce_plane_gmsd_scores) == 160, "the size include/ce_metrics.h states");

namespace {

template <class SAMPLE>
__global__ __launch_bounds__(kGmsdThreads) void k_plane_gmsd(const gmsd_args a)
{
    __shared__ gmsd_lds lds;
    __shared__ unsigned long long s_part[kGmsdWaves][kGmsdTerms];
    gmsd_stage<SAMPLE>(a, lds);
    __syncthreads();
    const gmsd_part t = gmsd_score(a, lds);
    unsigned long long v[kGmsdTerms] = {t.q, t.hh, t.hl, t.ll, t.max_dis};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] += __shfl_down(v[k], off, 64);
        const unsigned long long m = __shfl_down(v[4], off, 64);
        v[4] = m > v[4] ? m : v[4];
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < (int)kGmsdTerms; k++) s_part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < kGmsdTerms) {
        // at most 1024 positions of at most 2^32 each: the sums cannot wrap
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < (int)kGmsdWaves; k++) {
            const unsigned long long p = s_part[k][threadIdx.x];
            s = threadIdx.x == 4 ? (p > s ? p : s) : s + p;
        }
        const gmsd_where o = gmsd_tile(a);
        unsigned long long *acc = a.out + (size_t)o.pair * kGmsdOut + (size_t)o.plane * kGmsdTerms + threadIdx.x;
        if (o.live && s) {
            if (threadIdx.x == 4) atomicMax(acc, s);
            else atomicAdd(acc, s);
        }
    }
}

constexpr uint32_t kGridYMax = 65535;

}  // namespace

int ce_yuv_plane_gmsd(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs, const ce_yuv_image *tests,
                      uint32_t n_pairs, const uint32_t *pair_ref, ce_plane_gmsd_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    const auto bad = [ctx](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, "plane gmsd: " + why); };
    if (int rc = pf_check_pairs(ctx, "plane gmsd", refs, n_refs, tests, n_pairs, pair_ref, out)) return rc;
    const uint64_t w2 = ((uint64_t)width + 1) / 2, h2 = ((uint64_t)height + 1) / 2;
    if (w2 * h2 >= (1ull << 32))
        return bad("a luma plane of " + std::to_string(width) + " x " + std::to_string(height) + " has " + std::to_string(w2 * h2) +
                   " positions, 2^32 or more: the exact variance would not fit 128 bits");
    pf_images im;
    if (int rc = pf_check_images(ctx, "plane gmsd", width, height, refs, n_refs, tests, n_pairs, pair_ref, &im)) {
        // what the ingest's check of an image refuses carries the ingest's words: name the call in front of them
        if (ctx->err.rfind("plane gmsd: ", 0) != 0) ctx->err = "plane gmsd: " + ctx->err;
        return rc;
    }
    // luma has the most tiles; under 2^32 positions make under 2^31 tiles
    const uint64_t tiles = ((w2 + kGmsdTileW - 1) / kGmsdTileW) * ((h2 + kGmsdTileH - 1) / kGmsdTileH);
    if (tiles > 0x7fffffffull) return bad("more tiles than one launch covers");
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->pf_out_h.reserve(ctx, (size_t)kGmsdOut * n_pairs)) return rc;
    if (int rc = ctx->pf_out_d.reserve(ctx, (size_t)kGmsdOut * n_pairs)) return rc;
    if (int rc = pf_upload(ctx, im, refs, tests)) return rc;
    CE_HIP(ctx, hipMemsetAsync(ctx->pf_out_d.get(), 0, sizeof(unsigned long long) * kGmsdOut * n_pairs, ctx->stream));
    gmsd_args a{};
    a.tab = im.d_tab, a.pair_ref = im.d_pair_ref, a.out = ctx->pf_out_d;
    a.n_refs = n_refs, a.n_planes = im.n_planes, a.maxv = im.maxv;
    a.k = 24480ull << (2 * (im.depth - 8));
    for (uint32_t p = 0; p < im.n_planes; p++) a.w[p] = im.pw[p], a.h[p] = im.ph[p];
    // grid y is (pair, plane): at most 65535 a launch, whole pairs (plane_fidelity.hip: k_plane_sse)
    const uint32_t pairs_a_launch = kGridYMax / im.n_planes;
    for (uint32_t done = 0; done < n_pairs; done += pairs_a_launch) {
        const uint32_t count = std::min(n_pairs - done, pairs_a_launch);
        a.first = done;
        const dim3 grid((uint32_t)tiles, count * im.n_planes);
        if (im.bps == 1) CE_LAUNCH(ctx, "plane_gmsd_u8", k_plane_gmsd<uint8_t>, grid, dim3(kGmsdThreads), 0, a);
        else CE_LAUNCH(ctx, "plane_gmsd_u16", k_plane_gmsd<uint16_t>, grid, dim3(kGmsdThreads), 0, a);
    }
    CE_HIP(ctx, hipGetLastError());
    CE_HIP(ctx, hipMemcpyAsync(ctx->pf_out_h.get(), ctx->pf_out_d.get(), sizeof(unsigned long long) * kGmsdOut * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the caller's planes are free again
    for (uint32_t i = 0; i < n_pairs; i++) {
        const unsigned long long *r = ctx->pf_out_h.get() + (size_t)kGmsdOut * i;
        ce_plane_gmsd_scores s{};
        s.n_planes = im.n_planes;
        for (uint32_t p = 0; p < 3; p++) {
            s.gmsd[p] = s.gmsm[p] = NAN;
            if (p >= im.n_planes) continue;
            const gmsd_plane_result f = gmsd_finish(r + (size_t)p * kGmsdTerms, im.pw[p], im.ph[p]);
            s.sum_q[p] = f.sum_q, s.sum_q2[p][0] = f.sum_q2[0], s.sum_q2[p][1] = f.sum_q2[1], s.n_pos[p] = f.n_pos;
            s.gmsd[p] = f.gmsd, s.gmsm[p] = f.gmsm, s.max_dis[p] = f.max_dis;
        }
        out[i] = s;
    }
    return CE_OK;
}
