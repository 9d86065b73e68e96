// DSSIM on gfx950 — replaces rgb8_to_dssim_image + calculate_dssim
// (/root/reference/src/metrics/dssim.rs:102-114, 40-71 -> dssim_core::Dssim::{create_image, compare}).
//
// Per level (5 levels, each the 2x2 average of the previous in LINEAR RGB, floor sizes):
//   per image slot ("create_image", references once per reference, not once per pair):
//     linear RGB -> normalised L*a*b*  ->  chroma planes pre-blurred (= img);  references also: mu = blur(img),
//     sq = blur(img*img), kept per level for all their pairs (and across launches for a reference handle)
//   per pair ("compare"):
//     the distorted image's mu / sq and i12 = blur(img1*img2) -> SSIM map over the channel-averaged statistics
//   after the last level, for all levels at once: mean -> mean |avg - ssim| -> weighted score
// "blur" is the fixed 3x3 kernel applied twice with edge replication.  The per-level kernels are the streaming kernels of
// dssim_stream.hip (round 3; rounds 1-2 ran 32 x 32 LDS-tile kernels here: profiles/r03_experiments.md sections 1, 7); this
// file holds the tail reductions, the working set and the launch sequence.  Every plane op keeps the oracle's f32 operation
// order (oracle/dssim.c), so planes are bit-identical; sums are f64.  Build with -ffp-contract=off.
#include <algorithm>
#include <cstdlib>

#include "ce_internal.h"
#include "dssim_common.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ uint32_t slot_of(uint32_t z, uint32_t n_refs_used, uint32_t max_refs)
{
    return z < n_refs_used ? z : max_refs + (z - n_refs_used);
}

// ---- rgb8_to_dssim_image (dssim.rs:102-114): interleaved RGBA f32, a = 1.0 -------------------------
__global__ __launch_bounds__(TPB) void k_rgb8_to_rgba_f32(const uint8_t *__restrict__ rgb, const float *__restrict__ lut,
                                                          float4 *__restrict__ out, size_t n)
{
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB)
        out[i] = make_float4(s_lut[rgb[3 * i]], s_lut[rgb[3 * i + 1]], s_lut[rgb[3 * i + 2]], 1.0f);
}

__device__ __forceinline__ double block_sum(double v, double *s_red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < TPB / 64; k++) t += s_red[k];
    __syncthreads();
    return t;
}

// ---- the tail of every level in two launches (round 3: one avg + one absdev launch per LEVEL were ten of DSSIM's 21 dependent
// launches, each ~4.5 us on the critical path of a single-pair call) ------------------------------------------------------
struct ds_tail {
    uint32_t w[CE_DSSIM_SCALES], h[CE_DSSIM_SCALES], pitch[CE_DSSIM_SCALES], n_part[CE_DSSIM_SCALES], gx[CE_DSSIM_SCALES];
    uint32_t blk_end[CE_DSSIM_SCALES];  // absdev blocks of levels 0 .. l, running total (the launch's x extent is the last one)
    size_t plane[CE_DSSIM_SCALES], map_off[CE_DSSIM_SCALES];  // the level's SSIM maps start at map + map_off[l], one plane per pair
};

// avg = max(mean, 0)^(0.5^level): one block per (pair, level) reduces the compare kernel's partial sums in a fixed order
__global__ __launch_bounds__(TPB) void k_dssim_avg(const double *__restrict__ part, double *__restrict__ avg_out, ds_tail t, uint32_t n_levels,
                                                   uint32_t n_blocks)
{
    __shared__ double s_red[TPB];
    const uint32_t p = blockIdx.x, level = blockIdx.y;
    const double *pp = part + ((size_t)p * n_levels + level) * 2 * n_blocks;
    const uint32_t used_blocks = t.n_part[level];
    double v = 0.0;
    for (uint32_t k = threadIdx.x; k < used_blocks; k += TPB) v += pp[k];
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int off = TPB / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double avg = s_red[0] / (double)((size_t)t.w[level] * t.h[level]);
        if (!(avg > 0.0)) avg = 0.0;
        avg_out[(size_t)p * n_levels + level] = pow(avg, pow(0.5, (double)level));
    }
}

// mean absolute deviation of the SSIM map from avg; 1-D grid: per pair, the blocks of all levels one after the other
constexpr int AD_ROWS = 32;  // rows per block
__global__ __launch_bounds__(TPB) void k_dssim_absdev(const float *__restrict__ map, const double *__restrict__ avg_in,
                                                      double *__restrict__ part, ds_tail t, uint32_t n_levels, uint32_t n_blocks)
{
    __shared__ double s_red[TPB / 64];
    const uint32_t per_pair = t.blk_end[n_levels - 1], p = blockIdx.x / per_pair, bi = blockIdx.x % per_pair;
    uint32_t level = 0, first = 0;
#pragma unroll
    for (int l = 0; l + 1 < CE_DSSIM_SCALES; l++)
        if (l + 1 < (int)n_levels && bi >= t.blk_end[l]) level = l + 1, first = t.blk_end[l];
    const uint32_t w = t.w[level], h = t.h[level], pitch = t.pitch[level], gx = t.gx[level];
    const uint32_t bx = (bi - first) % gx, by = (bi - first) / gx;
    double *pp = part + ((size_t)p * n_levels + level) * 2 * n_blocks;
    const double avg = avg_in[(size_t)p * n_levels + level];
    const float *m = map + t.map_off[level] + (size_t)p * t.plane[level];
    // block = 64 columns x 32 rows, a thread walks 8 rows (stride 4): one block reduction per 2048 pixels
    const uint32_t x = bx * 64 + (threadIdx.x & 63);
    double val = 0.0;
#pragma unroll
    for (int k = 0; k < AD_ROWS / 4; k++) {
        const uint32_t y = by * AD_ROWS + 4 * k + (threadIdx.x >> 6);
        if (x < w && y < h) val += fabs(avg - (double)m[(size_t)y * pitch + x]);
    }
    const double s = block_sum(val, s_red);
    if (threadIdx.x == 0) pp[n_blocks + by * gx + bx] = s;
}

struct ds_geom {
    uint32_t npix[CE_DSSIM_SCALES];
    uint32_t nblk[CE_DSSIM_SCALES];
};

// one wave per pair: the per-block deviation sums of every level are added lane-strided and then across the wave
// (a fixed order, so the result is reproducible), lane 0 forms the level scores and the final value
__global__ __launch_bounds__(64) void k_dssim_finalize_pairs(const double *__restrict__ part, double *__restrict__ level_scores,
                                                             ce_dev_scores *__restrict__ scores, uint32_t n_pairs,
                                                             uint32_t n_levels, uint32_t n_blocks, ds_geom g)
{
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    if (p >= n_pairs) return;
    const double W[CE_DSSIM_SCALES] = {0.028, 0.197, 0.322, 0.298, 0.155};
    double ssim_sum = 0.0, weight_sum = 0.0;
    for (uint32_t l = 0; l < n_levels; l++) {
        const double *pp = part + (((size_t)p * n_levels + l) * 2 + 1) * n_blocks;
        double dev = 0.0;
        for (uint32_t k = lane; k < g.nblk[l]; k += 64) dev += pp[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dev += __shfl_down(dev, off, 64);
        dev = __shfl(dev, 0, 64);
        const double score = 1.0 - dev / (double)g.npix[l];
        if (lane == 0) level_scores[(size_t)p * CE_DSSIM_SCALES + l] = score;
        ssim_sum += score * W[l];
        weight_sum += W[l];
    }
    double ssim = ssim_sum / weight_sum;
    if (!(ssim > 2.220446049250313e-16)) ssim = 2.220446049250313e-16;
    if (lane == 0) scores[p].dssim = 1.0 / ssim - 1.0;
}

// level l's SSIM maps start at ds.map + map_offset(b, l): the levels one after the other, max_pairs planes each
size_t map_offset(const ce_batch *b, const ce_dssim_set &ds, int l)
{
    size_t off = 0;
    for (int k = 0; k < l; k++) off += (size_t)b->max_pairs * ds.lvl[k].plane;
    return off;
}
size_t map_offset(const ce_batch *b, int l) { return map_offset(b, b->ds, l); }

}  // namespace

static int dssim_prepare(ce_batch *b)
{
    if (b->ds.engaged()) return CE_OK;
    ce_ctx *ctx = b->ctx;
    ce_dssim_set D;
    uint32_t lw[CE_DSSIM_SCALES], lh[CE_DSSIM_SCALES];
    const int n = D.levels = (int)ce_plan_dssim_levels(b->w, b->h, CE_DSSIM_SCALES, lw, lh);  // make_scales_recursive (ce_plan.h)
    for (int l = 0; l < n; l++) {
        ce_plane_geom &d = D.lvl[l];
        d.w = lw[l];
        d.h = lh[l];
        d.pitch = (d.w + 31u) & ~31u;
        d.plane = (size_t)d.pitch * d.h;
    }
    const size_t slots = (size_t)b->max_refs + b->max_pairs, p0 = D.lvl[0].plane;
    // linear RGB ping-pong for levels >= 1 (level 0 is read from the u8 slabs): level l lives in lin[l & 1]
    const size_t p1 = n > 1 ? D.lvl[1].plane : 1;
    int rc = D.lin[0].alloc(ctx, slots * 3 * p1);
    if (rc == CE_OK) rc = D.lin[1].alloc(ctx, slots * 3 * p1);
    if (rc == CE_OK) rc = D.img.alloc(ctx, (size_t)b->max_pairs * 3 * p0);  // the distorted images' img, one level at a time
    // the references' planes, one set per level: they outlive the level loop (Dssim::create_image of the reference is
    // run once per reference, dssim.rs:54-59; kept across launches until a reference is written, ce_ref_state.h)
    for (int l = 0; l < n && rc == CE_OK; l++) {
        const size_t rn = (size_t)b->max_refs * 3 * D.lvl[l].plane;
        rc = D.rimg[l].alloc(ctx, rn);
        if (rc == CE_OK) rc = D.rmu[l].alloc(ctx, rn);
        if (rc == CE_OK) rc = D.rsq[l].alloc(ctx, rn);
    }
    // every level's SSIM maps, kept until the next launch (ce_dssim_read_maps)
    if (rc == CE_OK) rc = D.map.alloc(ctx, map_offset(b, D, n));
    // partial sums per (pair, level): the absdev kernel's blocks, or the compare kernel's strip tiles (>= 2 rows each)
    D.blocks = std::max(((D.lvl[0].w + 63) / 64) * ((D.lvl[0].h + AD_ROWS - 1) / AD_ROWS), ((D.lvl[0].w + CE_DSSIM_STRIP - 1) / CE_DSSIM_STRIP) * ((D.lvl[0].h + 1) / 2));
    if (rc == CE_OK) rc = D.part.alloc(ctx, (size_t)b->max_pairs * CE_DSSIM_SCALES * 2 * D.blocks);
    if (rc == CE_OK) rc = D.level_scores.alloc(ctx, (size_t)b->max_pairs * CE_DSSIM_SCALES);  // avg, then score
    if (rc != CE_OK) return rc;  // all or nothing: D releases what it got
    b->ds = std::move(D);
    return CE_OK;
}

int ce_launch_dssim(ce_batch *b, const uint8_t *d_refs, uint32_t n_refs_used, uint32_t n_pairs)
{
    ce_ctx *ctx = b->ctx;
    int rc = dssim_prepare(b);
    if (rc != CE_OK) return rc;
    // the references' img / mu / sq pyramid of an earlier launch is still valid?
    const bool cached = b->refs.reuse(CE_REF_DSSIM, d_refs, n_refs_used, 0);
    const uint32_t z0 = cached ? n_refs_used : 0;
    ds_geom g{};
    ds_tail tail{};
    for (int l = 0; l < b->ds.levels; l++) {
        const auto &d = b->ds.lvl[l];
        // create_image for every used slot (references once per reference), then compare per pair: dssim_stream.hip
        if ((rc = ce_dssim_create_stream(b, l, d_refs, n_refs_used, n_pairs, z0)) != CE_OK) return rc;
        uint32_t n_part = 0;
        if ((rc = ce_dssim_compare_stream(b, l, n_pairs, b->ds.map + map_offset(b, l), &n_part)) != CE_OK) return rc;
        tail.w[l] = d.w, tail.h[l] = d.h, tail.pitch[l] = d.pitch, tail.plane[l] = d.plane, tail.n_part[l] = n_part;
        tail.gx[l] = (d.w + 63) / 64;
        tail.map_off[l] = map_offset(b, l);
        g.npix[l] = d.w * d.h;
        g.nblk[l] = tail.gx[l] * ((d.h + AD_ROWS - 1) / AD_ROWS);
        tail.blk_end[l] = (l ? tail.blk_end[l - 1] : 0u) + g.nblk[l];
    }
    {
        const uint32_t nl = (uint32_t)b->ds.levels;
        CE_LAUNCH(ctx, "dssim_avg", k_dssim_avg, dim3(n_pairs, nl), dim3(TPB), 0, b->ds.part, b->ds.level_scores, tail, nl, b->ds.blocks);
        const dim3 gp(tail.blk_end[nl - 1] * n_pairs);
        CE_LAUNCH(ctx, "dssim_absdev", k_dssim_absdev, gp, dim3(TPB), 0, (const float *)b->ds.map, b->ds.level_scores, b->ds.part, tail, nl,
                  b->ds.blocks);
    }
    CE_LAUNCH(ctx, "dssim_finalize", k_dssim_finalize_pairs, dim3(n_pairs), dim3(64), 0, b->ds.part,
              b->ds.level_scores, b->d_scores, n_pairs, (uint32_t)b->ds.levels, b->ds.blocks, g);
    CE_HIP(ctx, hipGetLastError());
    if (!cached) b->refs.built(CE_REF_DSSIM, d_refs, n_refs_used, 0);
    return CE_OK;
}

// SsimMap of pairs [first, first + count) at `level`, from the last launch: the maps (B = 1) or their B x B cell minima
// into `maps` and the level scores into `ssim`, either of them may be null; the caller has checked the arguments.
// Enqueued on the context's stream behind that launch (maps.hip: ce_read_map_cells) and waited for.
int ce_dssim_read_maps(ce_batch *b, uint32_t level, uint32_t first, uint32_t count, uint32_t block, float *maps, double *ssim)
{
    ce_ctx *ctx = b->ctx;
    if (ssim) {  // every pair's score of this level: a strided gather out of [pair][CE_DSSIM_SCALES]
        CE_HIP(ctx, hipMemcpy2DAsync(ssim, sizeof(double), b->ds.level_scores + (size_t)first * CE_DSSIM_SCALES + level,
                                     CE_DSSIM_SCALES * sizeof(double), sizeof(double), count, hipMemcpyDeviceToHost, ctx->stream));
        if (!maps) CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (!maps) return CE_OK;
    const auto &d = b->ds.lvl[level];
    return ce_read_map_cells(b, "dssim_block_min", b->ds.map + map_offset(b, (int)level), d, first, count, block, true, b->ds.cells, maps);
}

int ce_launch_rgb8_to_dssim_image(ce_ctx *ctx, const uint8_t *d_rgb, float *d_rgba, size_t n_pixels)
{
    if (n_pixels == 0) return CE_OK;
    size_t blocks = std::min<size_t>((n_pixels + TPB - 1) / TPB, 4096);
    CE_LAUNCH(ctx, "rgb8_to_dssim_image", k_rgb8_to_rgba_f32, dim3((uint32_t)blocks), dim3(TPB), 0, d_rgb, ctx->d_lut_powf,
              reinterpret_cast<float4 *>(d_rgba), n_pixels);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
