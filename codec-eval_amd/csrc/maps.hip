// Readout of per-pair maps kept on the device: Butteraugli's diffmaps (CE_FLAG_BUTTERAUGLI_DIFFMAP, butteraugli.hip),
// DSSIM's per-level SSIM maps (dssim.hip) and SSIMULACRA2's per-scale error maps (CE_FLAG_SSIMULACRA2_MAPS, ssim2.hip).
// All are [pair][h][pitch] float planes, a pair's plane `plane` floats after the previous one's; a readout packs pairs
// [first, first + count) to the host, whole (B = 1) or as the max / min of every B x B cell.
#include "ce_internal.h"

namespace {

struct reduce_max {
    static __device__ __forceinline__ float identity() { return -__builtin_inff(); }
    static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
};
struct reduce_min {
    static __device__ __forceinline__ float identity() { return __builtin_inff(); }
    static __device__ __forceinline__ float op(float a, float b) { return fminf(a, b); }
};

// B x B cell reductions (B = 1 << lb, 2 .. 64) of the maps of pairs [first, first + count), packed
// [count][ceil(h / B)][ceil(w / B)].  One thread per column of one cell row: the reduction down the cell's rows (a wave
// reads 64 adjacent columns of a row), then across the cell's B lanes (B <= 64: a cell never leaves its wave).  Columns at
// or past w enter as the identity and read nothing, so the pitch padding is never read; max and min of the same floats
// are exact.
template <class R>
__global__ __launch_bounds__(256) void k_map_block_reduce(const float *__restrict__ map, ce_plane_geom g, uint32_t first, uint32_t lb,
                                                          uint32_t tiles_x, uint32_t bw, uint32_t bh, float *__restrict__ out)
{
    const uint32_t t = blockIdx.x % tiles_x, cy = (blockIdx.x / tiles_x) % bh, q = blockIdx.x / tiles_x / bh;
    const uint32_t B = 1u << lb, x = t * 256 + threadIdx.x;
    float m = R::identity();
    if (x < g.w) {
        const float *col = map + (size_t)(first + q) * g.plane + x;
        const uint32_t y1 = min((cy + 1) << lb, g.h);
        for (uint32_t y = cy << lb; y < y1; y++) m = R::op(m, col[(size_t)y * g.pitch]);
    }
    for (uint32_t off = 1; off < B; off <<= 1) m = R::op(m, __shfl_xor(m, (int)off, 64));
    if (x < g.w && (x & (B - 1)) == 0) out[((size_t)q * bh + cy) * bw + (x >> lb)] = m;
}

}  // namespace

// The maps of pairs [first, first + count) of `map` (geometry g) into `out` (host, count * ceil(h / B) * ceil(w / B)
// floats): B = 1 the maps themselves, else the cell max (take_min false) or min (take_min true), reduced into the grow-only
// device buffer `cells`.  The caller has checked the range and B.  Enqueued on the context's stream, behind the launch that
// wrote the maps (a forked metric chain joins that stream before the launch returns), and waited for.
int ce_read_map_cells(ce_batch *b, const char *name, const float *map, ce_plane_geom g, uint32_t first, uint32_t count, uint32_t block,
                      bool take_min, ce_dev<float> &cells, float *out)
{
    ce_ctx *ctx = b->ctx;
    if (block == 1 && g.plane == (size_t)g.pitch * g.h) {  // [pair][h][pitch] rows are contiguous over the pairs: one pitched copy
        CE_HIP(ctx, hipMemcpy2DAsync(out, (size_t)g.w * sizeof(float), map + (size_t)first * g.plane, (size_t)g.pitch * sizeof(float),
                                     (size_t)g.w * sizeof(float), (size_t)count * g.h, hipMemcpyDeviceToHost, ctx->stream));
        CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CE_OK;
    }
    if (block == 1) {  // padded rows or other planes between the pairs' maps (SSIMULACRA2): one pitched copy per pair
        for (uint32_t q = 0; q < count; q++)
            CE_HIP(ctx, hipMemcpy2DAsync(out + (size_t)q * g.w * g.h, (size_t)g.w * sizeof(float), map + (size_t)(first + q) * g.plane,
                                         (size_t)g.pitch * sizeof(float), (size_t)g.w * sizeof(float), g.h, hipMemcpyDeviceToHost,
                                         ctx->stream));
        CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CE_OK;
    }
    uint32_t lb = 0;
    while ((1u << lb) < block) lb++;
    const uint32_t bw = (g.w + block - 1) >> lb, bh = (g.h + block - 1) >> lb, tiles_x = (g.w + 255) / 256;
    const size_t n = (size_t)count * bw * bh;
    if (int rc = cells.reserve(ctx, n)) return rc;
    const size_t blocks = (size_t)tiles_x * bh * count;
    if (blocks > 0x7fffffffu) {
        ctx->err = "map readout too large for one launch";
        return CE_ERR_INVALID_ARG;
    }
    if (take_min)
        CE_LAUNCH_ON(ctx, ctx->stream, name, k_map_block_reduce<reduce_min>, dim3((uint32_t)blocks), dim3(256), 0, map, g, first, lb,
                     tiles_x, bw, bh, cells.get());
    else
        CE_LAUNCH_ON(ctx, ctx->stream, name, k_map_block_reduce<reduce_max>, dim3((uint32_t)blocks), dim3(256), 0, map, g, first, lb,
                     tiles_x, bw, bh, cells.get());
    CE_HIP(ctx, hipGetLastError());
    CE_HIP(ctx, hipMemcpyAsync(out, cells.get(), n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CE_OK;
}
