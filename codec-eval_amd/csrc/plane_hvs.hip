// PSNR-HVS and PSNR-HVS-M of a decoder's Y'CbCr planes (include/ce_metrics.h: ce_yuv_plane_hvs): per
// pair and plane the exact sums of the quantised, CSF-weighted squared DCT differences, without and with Ponomarenko's
// contrast mask, which the host finishes in f64.  One kernel, k_plane_hvs, over (groups of 32 DCT blocks, pairs x planes) in
// one launch as k_plane_sse shares its launch among the planes: eight lanes a DCT block, the three phases of
// plane_hvs_kernel.h between two barriers, then the thread block's two integers reduced as k_plane_sse reduces its one -
// shuffles, LDS across the waves - and handed over as their low and high 32 bits with two vector atomics each, so that
// neither accumulator can wrap at any image size.  The planes are read where they lie through plane_fidelity_kernel.h's
// table; the checks and the upload are plane_images.h's, shared with ce_yuv_plane_fidelity.  The device code is
// plane_hvs_kernel.h's, which a test also compiles for the host.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ce_internal.h"

#include "plane_hvs_kernel.h"

#include "plane_images.h"

namespace {

template <class SAMPLE>
__global__ __launch_bounds__(kHvsThreads) void k_plane_hvs(const hvs_args a)
{
    __shared__ hvs_lds lds;
    __shared__ unsigned long long s_part[kHvsWaves][2];
    hvs_rows<SAMPLE>(a, lds);
    __syncthreads();
    hvs_cols col;
    hvs_columns(a, lds, col);
    __syncthreads();
    unsigned long long q[2];
    hvs_score(a, lds, col, q);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        q[0] += __shfl_down(q[0], off, 64);
        q[1] += __shfl_down(q[1], off, 64);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][0] = q[0], s_part[threadIdx.x >> 6][1] = q[1];
    __syncthreads();
    if (threadIdx.x < 2) {
        // at most 32 DCT blocks of under 2^44.7 each: the sum cannot wrap
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < (int)kHvsWaves; k++) t += s_part[k][threadIdx.x];
        const hvs_where o = hvs_block(a);
        unsigned long long *acc = a.out + (size_t)o.pair * kHvsOut + ((size_t)o.plane * 2 + threadIdx.x) * 2;
        if (t & 0xffffffffull) atomicAdd(acc, t & 0xffffffffull);
        if (t >> 32) atomicAdd(acc + 1, t >> 32);
    }
}

constexpr uint32_t kGridYMax = 65535;

// JPEG (ITU-T T.81) Annex K, table K.1, in natural order
const int kAnnexK[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                         14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                         49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};

uint64_t blocks_of(uint32_t pw, uint32_t ph, uint32_t step)
{
    return pw < 8 || ph < 8 ? 0 : (uint64_t)((pw - 8) / step + 1) * ((ph - 8) / step + 1);
}

double finish(const unsigned long long acc[2], uint64_t n_blocks, uint32_t depth)
{
    if (acc[0] == 0 && acc[1] == 0) return INFINITY;
    const double maxv = (double)((1u << depth) - 1u);
    const double s = (((double)acc[1] * 4294967296.0 + (double)acc[0]) / (double)(1ull << (36 - 2 * depth))) / (64.0 * (double)n_blocks);
    return 10.0 * std::log10(maxv * maxv / s);
}

}  // namespace

int ce_yuv_plane_hvs(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs, const ce_yuv_image *tests,
                     uint32_t n_pairs, const uint32_t *pair_ref, uint32_t step, ce_plane_hvs_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    const auto bad = [ctx](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, "plane hvs: " + why); };
    if (int rc = pf_check_pairs(ctx, "plane hvs", refs, n_refs, tests, n_pairs, pair_ref, out)) return rc;
    if (step < 1 || step > 8) return bad("step must be 1 .. 8 samples from a block to the next, got " + std::to_string(step));
    pf_images im;
    if (int rc = pf_check_images(ctx, "plane hvs", width, height, refs, n_refs, tests, n_pairs, pair_ref, &im)) return rc;
    if (width < 8 || height < 8) return bad("a luma plane of " + std::to_string(width) + " x " + std::to_string(height) + " holds no 8 x 8 block");
    uint64_t n_blocks[3] = {};
    for (uint32_t p = 0; p < im.n_planes; p++) n_blocks[p] = blocks_of(im.pw[p], im.ph[p], step);
    const uint64_t groups = (n_blocks[0] + kHvsBlocks - 1) / kHvsBlocks;  // luma has the most blocks
    if (groups > 0x7fffffffull) return bad("more DCT blocks than one launch covers");
    // the tables: single f64 divisions
    double tables[128];
    for (int i = 0; i < 64; i++) tables[i] = 25.73509 / (double)kAnnexK[i], tables[64 + i] = 100.0 / (double)(kAnnexK[i] * kAnnexK[i]);
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->pf_out_h.reserve(ctx, (size_t)kHvsOut * n_pairs)) return rc;
    if (int rc = ctx->pf_out_d.reserve(ctx, (size_t)kHvsOut * n_pairs)) return rc;
    if (int rc = pf_upload(ctx, im, refs, tests, tables, sizeof(tables))) return rc;
    CE_HIP(ctx, hipMemsetAsync(ctx->pf_out_d.get(), 0, sizeof(unsigned long long) * kHvsOut * n_pairs, ctx->stream));
    hvs_args a{};
    a.tab = im.d_tab, a.pair_ref = im.d_pair_ref, a.out = ctx->pf_out_d;
    a.csf = reinterpret_cast<const double *>(im.d_extra), a.mc = a.csf + 64;
    a.n_refs = n_refs, a.n_planes = im.n_planes, a.maxv = im.maxv, a.step = step;
    a.unit = (double)(1ull << (36 - 2 * im.depth));
    for (uint32_t p = 0; p < im.n_planes; p++) a.w[p] = im.pw[p], a.h[p] = im.ph[p];
    // grid y is (pair, plane): at most 65535 a launch, whole pairs (plane_fidelity.hip: k_plane_sse)
    const uint32_t pairs_a_launch = kGridYMax / im.n_planes;
    for (uint32_t done = 0; done < n_pairs; done += pairs_a_launch) {
        const uint32_t count = std::min(n_pairs - done, pairs_a_launch);
        a.first = done;
        const dim3 grid((uint32_t)groups, count * im.n_planes);
        if (im.bps == 1) CE_LAUNCH(ctx, "plane_hvs_u8", k_plane_hvs<uint8_t>, grid, dim3(kHvsThreads), 0, a);
        else CE_LAUNCH(ctx, "plane_hvs_u16", k_plane_hvs<uint16_t>, grid, dim3(kHvsThreads), 0, a);
    }
    CE_HIP(ctx, hipGetLastError());
    CE_HIP(ctx, hipMemcpyAsync(ctx->pf_out_h.get(), ctx->pf_out_d.get(), sizeof(unsigned long long) * kHvsOut * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the caller's planes are free again
    for (uint32_t i = 0; i < n_pairs; i++) {
        const unsigned long long *r = ctx->pf_out_h.get() + (size_t)kHvsOut * i;
        ce_plane_hvs_scores s{};
        s.n_planes = im.n_planes, s.step = step;
        for (uint32_t p = 0; p < 3; p++) {
            s.psnr_hvs[p] = s.psnr_hvsm[p] = NAN;
            if (p >= im.n_planes || n_blocks[p] == 0) continue;
            s.n_blocks[p] = n_blocks[p];
            for (int m = 0; m < 2; m++) {
                // the accumulators as the thread blocks left them -> the sum's low 32 bits and the rest: whatever the grid, one pair of integers
                const unsigned long long *acc = r + ((size_t)p * 2 + m) * 2;
                unsigned long long q[2] = {acc[0] & 0xffffffffull, acc[1] + (acc[0] >> 32)};
                (m ? s.hvsm_q : s.hvs_q)[p][0] = q[0], (m ? s.hvsm_q : s.hvs_q)[p][1] = q[1];
                (m ? s.psnr_hvsm : s.psnr_hvs)[p] = finish(q, n_blocks[p], im.depth);
            }
        }
        out[i] = s;
    }
    return CE_OK;
}
