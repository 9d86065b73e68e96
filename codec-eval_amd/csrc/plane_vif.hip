// Pixel-domain VIF of a decoder's Y'CbCr planes (include/ce_metrics.h: ce_yuv_plane_vif): per pair, plane
// and scale the exact sums of the quantised information terms of the test and of the reference, which the host finishes in
// f64.  Two kernels, each instantiated per window length and source.  k_vif_stats, over (tiles, pairs x planes) of one scale in
// one launch, is k_plane_level's shape with N taps: the tile of both sides staged into LDS - scale 1 from the planes where they
// lie, through plane_fidelity_kernel.h's table, scales 2 - 4 from the context's f64 pyramid - the five streams filtered down
// the columns into LDS and along the rows, the per-position text, then the thread block's two integers reduced as k_plane_sse
// reduces its one and added with a vector atomic each.  k_vif_reduce, over (tiles of 16 x 16 outputs, images x planes), writes
// the next scale through the same three phases: the filter's outputs at even rows and columns only, once per image - a
// reference that several pairs name is reduced once.
// Integer sums do not depend on the order, so the scores do not depend on the grid.  The checks and the upload are
// plane_images.h's, shared with the other plane calls.  The device code is plane_vif_kernel.h's, which a test also compiles for
// the host.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ce_internal.h"

#include "plane_vif_kernel.h"

#include "plane_images.h"

static_assert(sizeof(ce_plane_vif_scores) == 424, "the size include/ce_metrics.h states");

namespace {

template <int N, class SAMPLE>
__global__ __launch_bounds__(kVifThreads) void k_vif_stats(const vif_args a)
{
    using G = vif_geom<N>;
    __shared__ vif_stage_t<SAMPLE> s_in[2 * G::in_len];
    __shared__ __attribute__((aligned(16))) double s_col[kVifStreams * G::col_len];
    __shared__ unsigned long long s_part[kVifWaves][2];
    vif_stage<N, SAMPLE>(a, s_in);
    __syncthreads();
    vif_columns<N>(a, s_in, s_col);
    __syncthreads();
    unsigned long long acc[2];
    vif_lane<N>(a, s_col, acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc[0] += __shfl_down(acc[0], off, 64);
        acc[1] += __shfl_down(acc[1], off, 64);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][0] = acc[0], s_part[threadIdx.x >> 6][1] = acc[1];
    __syncthreads();
    if (threadIdx.x < 2) {
        // 1024 positions of under 2^28 each
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < (int)kVifWaves; k++) t += s_part[k][threadIdx.x];
        const vif_where o = vif_block<N>(a);
        if (t) atomicAdd(a.out + (size_t)o.pair * kVifOut + ((size_t)o.plane * kVifScales + a.scale) * 2 + threadIdx.x, t);
    }
}

template <int N, class SAMPLE>
__global__ __launch_bounds__(kVifThreads) void k_vif_reduce(const vif_reduce_args a)
{
    using G = vif_reduce_geom<N>;
    __shared__ vif_stage_t<SAMPLE> s_in[G::in_len];
    __shared__ double s_col[G::col_len];
    vif_reduce_stage<N, SAMPLE>(a, s_in);
    __syncthreads();
    vif_reduce_columns<N>(a, s_in, s_col);
    __syncthreads();
    vif_reduce_rows<N>(a, s_col);
}

constexpr uint32_t kGridYMax = 65535;

// what the call has worked out about its planes: sizes per scale, and where each scale of each plane lies in the pyramid
struct vif_job {
    uint32_t w[3][kVifScales] = {}, h[3][kVifScales] = {};  // 0 where the plane does not run
    size_t off[3][kVifScales] = {};                         // doubles; scales 2 - 4
    bool ran[3] = {};
};

// scale s (1 .. 3) of images [first, first + count) from scale s - 1
int reduce_run(ce_ctx *ctx, const pf_images &im, const vif_job &j, double *pyr, uint32_t s, uint32_t first, uint32_t count)
{
    vif_reduce_args q{};
    q.tab = im.d_tab, q.src = pyr, q.dst = pyr, q.n_planes = im.n_planes, q.maxv = im.maxv;
    q.unit = 1.0 / (double)(1u << (im.depth - 8));
    for (uint32_t p = 0; p < im.n_planes; p++) {
        q.w[p] = j.w[p][s - 1], q.h[p] = j.h[p][s - 1], q.ow[p] = j.w[p][s], q.oh[p] = j.h[p][s];
        q.src_off[p] = j.off[p][s - 1], q.dst_off[p] = j.off[p][s];
    }
    // luma has the most tiles
    const uint32_t bx = ((q.ow[0] + kVifReduceTile - 1) / kVifReduceTile) * ((q.oh[0] + kVifReduceTile - 1) / kVifReduceTile);
    const uint32_t images_a_launch = kGridYMax / im.n_planes;
    for (uint32_t done = 0; done < count; done += images_a_launch) {
        q.first = first + done;
        const dim3 grid(bx, std::min(count - done, images_a_launch) * im.n_planes);
        if (s == 1 && im.bps == 1) CE_LAUNCH(ctx, "vif_reduce_9_u8", (k_vif_reduce<9, uint8_t>), grid, dim3(kVifThreads), 0, q);
        else if (s == 1) CE_LAUNCH(ctx, "vif_reduce_9_u16", (k_vif_reduce<9, uint16_t>), grid, dim3(kVifThreads), 0, q);
        else if (s == 2) CE_LAUNCH(ctx, "vif_reduce_5_f64", (k_vif_reduce<5, double>), grid, dim3(kVifThreads), 0, q);
        else CE_LAUNCH(ctx, "vif_reduce_3_f64", (k_vif_reduce<3, double>), grid, dim3(kVifThreads), 0, q);
    }
    return CE_OK;
}

double ratio(uint64_t num, uint64_t den) { return den == 0 ? 1.0 : (double)num / (double)den; }

}  // namespace

extern "C" int ce_vif_window(uint32_t scale, double *out)
{
    if (!out) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_vif_window: null pointer");
    if (scale < 1 || scale > (uint32_t)kVifScales) return ce_fail(nullptr, CE_ERR_INVALID_ARG, "ce_vif_window: scale must be 1 .. 4");
    for (int i = 0; i < vif_taps((int)scale - 1); i++)
        out[i] = scale == 1 ? vif_g<17>(i) : scale == 2 ? vif_g<9>(i) : scale == 3 ? vif_g<5>(i) : vif_g<3>(i);
    return CE_OK;
}

int ce_yuv_plane_vif(ce_ctx *ctx, uint32_t width, uint32_t height, const ce_yuv_image *refs, uint32_t n_refs, const ce_yuv_image *tests,
                     uint32_t n_pairs, const uint32_t *pair_ref, ce_plane_vif_scores *out)
{
    if (!ctx) return CE_ERR_INVALID_ARG;
    const auto bad = [ctx](const std::string &why) { return ce_fail(ctx, CE_ERR_INVALID_ARG, "plane vif: " + why); };
    if (int rc = pf_check_pairs(ctx, "plane vif", refs, n_refs, tests, n_pairs, pair_ref, out)) return rc;
    pf_images im;
    if (int rc = pf_check_images(ctx, "plane vif", width, height, refs, n_refs, tests, n_pairs, pair_ref, &im)) return rc;
    if (width < 41 || height < 41)
        return bad("a luma plane of " + std::to_string(width) + " x " + std::to_string(height) + " is under 41 x 41: it leaves scale 4 no position");
    const size_t n_img = (size_t)n_refs + n_pairs;
    vif_job j;
    size_t pyr = 0;
    for (uint32_t p = 0; p < im.n_planes; p++) {
        if (!(j.ran[p] = im.pw[p] >= 41 && im.ph[p] >= 41)) continue;
        uint32_t w = im.pw[p], h = im.ph[p];
        for (int s = 0; s < kVifScales; s++) {
            if (s) {
                w = (w - vif_taps(s) + 2) / 2, h = (h - vif_taps(s) + 2) / 2;
                j.off[p][s] = pyr, pyr += n_img * w * h;
            }
            j.w[p][s] = w, j.h[p][s] = h;
        }
    }
    // scratch: the pyramid and the results here; the planes and the tables in pf_upload (plane_images.h)
    CE_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->pf_vif_pyr.reserve(ctx, pyr)) return rc;
    if (int rc = ctx->pf_out_h.reserve(ctx, (size_t)kVifOut * n_pairs)) return rc;
    if (int rc = ctx->pf_out_d.reserve(ctx, (size_t)kVifOut * n_pairs)) return rc;
    if (int rc = pf_upload(ctx, im, refs, tests)) return rc;
    CE_HIP(ctx, hipMemsetAsync(ctx->pf_out_d.get(), 0, sizeof(unsigned long long) * kVifOut * n_pairs, ctx->stream));
    // the references the pairs name, as runs of consecutive images: each is reduced once (plane_fidelity.hip: launch)
    std::vector<bool> named(n_refs, false);
    for (uint32_t i = 0; i < n_pairs; i++) named[im.ref_of[i]] = true;
    std::vector<std::pair<uint32_t, uint32_t>> runs;  // first, count
    for (uint32_t r = 0; r < n_refs; r++)
        if (named[r]) {
            if (!runs.empty() && runs.back().first + runs.back().second == r) runs.back().second++;
            else runs.emplace_back(r, 1u);
        }
    vif_args a{};
    a.tab = im.d_tab, a.pyr = ctx->pf_vif_pyr, a.pair_ref = im.d_pair_ref, a.out = ctx->pf_out_d;
    a.n_refs = n_refs, a.n_planes = im.n_planes, a.maxv = im.maxv;
    a.unit = 1.0 / (double)(1u << (im.depth - 8));
    // grid y is (pair, plane): at most 65535 a launch, whole pairs (plane_hvs.hip)
    const uint32_t pairs_a_launch = kGridYMax / im.n_planes;
    for (uint32_t s = 0; s < (uint32_t)kVifScales; s++) {
        if (s) {
            for (const auto &run : runs)
                if (int rc = reduce_run(ctx, im, j, ctx->pf_vif_pyr, s, run.first, run.second)) return rc;
            if (int rc = reduce_run(ctx, im, j, ctx->pf_vif_pyr, s, n_refs, n_pairs)) return rc;  // the tests
        }
        a.scale = s;
        for (uint32_t p = 0; p < im.n_planes; p++) a.w[p] = j.w[p][s], a.h[p] = j.h[p][s], a.off[p] = j.off[p][s];
        const uint32_t taps = (uint32_t)vif_taps((int)s);  // luma has the most tiles
        const uint64_t tiles = (uint64_t)((j.w[0][s] - taps + kVifTileW) / kVifTileW) * ((j.h[0][s] - taps + kVifTileH) / kVifTileH);
        if (tiles > 0x7fffffffull) return bad("more tiles than one launch covers");
        for (uint32_t done = 0; done < n_pairs; done += pairs_a_launch) {
            a.first = done;
            const dim3 grid((uint32_t)tiles, std::min(n_pairs - done, pairs_a_launch) * im.n_planes);
            if (s == 0 && im.bps == 1) CE_LAUNCH(ctx, "vif_stats_17_u8", (k_vif_stats<17, uint8_t>), grid, dim3(kVifThreads), 0, a);
            else if (s == 0) CE_LAUNCH(ctx, "vif_stats_17_u16", (k_vif_stats<17, uint16_t>), grid, dim3(kVifThreads), 0, a);
            else if (s == 1) CE_LAUNCH(ctx, "vif_stats_9_f64", (k_vif_stats<9, double>), grid, dim3(kVifThreads), 0, a);
            else if (s == 2) CE_LAUNCH(ctx, "vif_stats_5_f64", (k_vif_stats<5, double>), grid, dim3(kVifThreads), 0, a);
            else CE_LAUNCH(ctx, "vif_stats_3_f64", (k_vif_stats<3, double>), grid, dim3(kVifThreads), 0, a);
        }
    }
    CE_HIP(ctx, hipGetLastError());
    CE_HIP(ctx, hipMemcpyAsync(ctx->pf_out_h.get(), ctx->pf_out_d.get(), sizeof(unsigned long long) * kVifOut * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the caller's planes are free again
    for (uint32_t i = 0; i < n_pairs; i++) {
        const unsigned long long *r = ctx->pf_out_h.get() + (size_t)kVifOut * i;
        ce_plane_vif_scores v{};
        v.n_planes = im.n_planes;
        for (uint32_t p = 0; p < 3; p++) {
            v.vifp[p] = NAN;
            for (int s = 0; s < kVifScales; s++) v.vif_scale[p][s] = NAN;
            if (p >= im.n_planes || !j.ran[p]) continue;
            v.ran[p] = 1;
            uint64_t num = 0, den = 0;
            for (int s = 0; s < kVifScales; s++) {
                const uint32_t taps = (uint32_t)vif_taps(s);
                v.num_q[p][s] = r[((size_t)p * kVifScales + s) * 2], v.den_q[p][s] = r[((size_t)p * kVifScales + s) * 2 + 1];
                v.n_pos[p][s] = (uint64_t)(j.w[p][s] - taps + 1) * (j.h[p][s] - taps + 1);
                v.vif_scale[p][s] = ratio(v.num_q[p][s], v.den_q[p][s]);
                num += v.num_q[p][s], den += v.den_q[p][s];
            }
            v.vifp[p] = ratio(num, den);
        }
        out[i] = v;
    }
    return CE_OK;
}
