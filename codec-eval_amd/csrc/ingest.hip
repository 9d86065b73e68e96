// Decoded-image ingest on the device: the per-pixel host passes the reference runs
// between a decoder and the metrics become one streaming kernel that writes the packed RGB8 slab slot.
//   RGBA8  -> RGB8 : ImageData::to_rgb8_vec, src/eval/session.rs:98-117 (alpha dropped)
//   RGB16 / RGBA16 holding 10-bit samples -> RGB8 : to_8bit, crates/codec-iter/src/avif_config.rs:122-125
//                                                   ((v * 255 + 512) / 1023).min(255), integer, bit-exact
#include "ce_internal.h"

namespace {

__device__ __forceinline__ uint8_t to_8bit(uint32_t v)
{
    const uint32_t q = (v * 255u + 512u) / 1023u;
    return (uint8_t)(q < 255u ? q : 255u);
}

// one pixel per thread; writes go out as bytes (3 B/px), reads are 4 or 8 B per pixel
template <int FORMAT>
__global__ __launch_bounds__(256) void k_ingest(const void *__restrict__ src, uint8_t *__restrict__ dst, size_t n_pixels)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x * blockDim.x) {
        uint8_t r, g, b;
        if (FORMAT == CE_PIXEL_RGBA8) {
            const uchar4 p = reinterpret_cast<const uchar4 *>(src)[i];
            r = p.x, g = p.y, b = p.z;
        } else if (FORMAT == CE_PIXEL_RGB16_10BIT) {
            const uint16_t *p = reinterpret_cast<const uint16_t *>(src) + 3 * i;
            r = to_8bit(p[0]), g = to_8bit(p[1]), b = to_8bit(p[2]);
        } else {
            const ushort4 p = reinterpret_cast<const ushort4 *>(src)[i];
            r = to_8bit(p.x), g = to_8bit(p.y), b = to_8bit(p.z);
        }
        dst[3 * i] = r;
        dst[3 * i + 1] = g;
        dst[3 * i + 2] = b;
    }
}

// ---- deep ingest (include/ce_metrics.h: ce_batch_create_deep) ---------------------------------------------------------
// A decoder's samples -> the packed u16 RGB slab of a deep batch, one read and one write per sample: RGB16 / RGBA16 (alpha
// dropped) clamped to maxv = 2^depth - 1 as to_8bit's .min does, RGB8 / RGBA8 widened (depth 8 only).  A thread takes
// eight pixels where the slab slot is 16-byte aligned: 48 bytes out as three 16-byte stores (a group starts at a multiple of
// 48 bytes), the source in 16-byte loads where its pixel size allows it (RGB16: three, RGBA16:
// four, RGBA8: two); RGB8's 24 bytes come as three 8-byte loads.  The tail of fewer than eight pixels, and a slot that is
// not 16-byte aligned, go sample by sample.
template <int FORMAT>
__global__ __launch_bounds__(256) void k_ingest_deep(const void *__restrict__ src, uint16_t *__restrict__ dst, size_t n_pixels, uint32_t maxv)
{
    // slot k of a slab starts at k * w * h * 6 bytes: 16-byte aligned or not, the same for the whole launch
    const size_t n_groups = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? n_pixels / 8 : 0;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    auto clamp2 = [maxv](uint32_t v) {  // two packed samples
        const uint32_t lo = min(v & 0xffffu, maxv), hi = min(v >> 16, maxv);
        return lo | (hi << 16);
    };
    for (size_t gi = tid; gi < n_groups; gi += nthreads) {
        uint32_t o[12];  // 24 samples
        if (FORMAT == CE_PIXEL_RGB16) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src) + 3 * gi;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint4 v = s4[k];
                o[4 * k] = clamp2(v.x), o[4 * k + 1] = clamp2(v.y), o[4 * k + 2] = clamp2(v.z), o[4 * k + 3] = clamp2(v.w);
            }
        } else if (FORMAT == CE_PIXEL_RGBA16) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src) + 4 * gi;
#pragma unroll
            for (int k = 0; k < 2; k++) {  // four pixels (r g | b a) x 4 -> six dwords
                const uint4 p = s4[2 * k], q = s4[2 * k + 1];
                const uint32_t rg0 = clamp2(p.x), b0 = min(p.y & 0xffffu, maxv), rg1 = clamp2(p.z), b1 = min(p.w & 0xffffu, maxv);
                const uint32_t rg2 = clamp2(q.x), b2 = min(q.y & 0xffffu, maxv), rg3 = clamp2(q.z), b3 = min(q.w & 0xffffu, maxv);
                o[6 * k] = rg0, o[6 * k + 1] = b0 | (rg1 << 16), o[6 * k + 2] = (rg1 >> 16) | (b1 << 16);
                o[6 * k + 3] = rg2, o[6 * k + 4] = b2 | (rg3 << 16), o[6 * k + 5] = (rg3 >> 16) | (b3 << 16);
            }
        } else if (FORMAT == CE_PIXEL_RGBA8) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src) + 2 * gi;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const uint4 v = s4[k];
                const uint32_t px[4] = {v.x, v.y, v.z, v.w};
                uint32_t smp[12];
#pragma unroll
                for (int j = 0; j < 4; j++) smp[3 * j] = px[j] & 255u, smp[3 * j + 1] = (px[j] >> 8) & 255u, smp[3 * j + 2] = (px[j] >> 16) & 255u;
#pragma unroll
                for (int j = 0; j < 6; j++) o[6 * k + j] = smp[2 * j] | (smp[2 * j + 1] << 16);
            }
        } else {  // CE_PIXEL_RGB8: 24 bytes, 8-byte aligned
            const uint2 *s2 = reinterpret_cast<const uint2 *>(src) + 3 * gi;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint2 v = s2[k];
                o[4 * k] = (v.x & 255u) | (((v.x >> 8) & 255u) << 16), o[4 * k + 1] = ((v.x >> 16) & 255u) | ((v.x >> 24) << 16);
                o[4 * k + 2] = (v.y & 255u) | (((v.y >> 8) & 255u) << 16), o[4 * k + 3] = ((v.y >> 16) & 255u) | ((v.y >> 24) << 16);
            }
        }
        uint4 *d4 = reinterpret_cast<uint4 *>(dst) + 3 * gi;
#pragma unroll
        for (int k = 0; k < 3; k++) d4[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
    // the last n_pixels % 8 pixels
    for (size_t i = n_groups * 8 + tid; i < n_pixels; i += nthreads) {
        uint32_t r, g, b;
        if (FORMAT == CE_PIXEL_RGB16 || FORMAT == CE_PIXEL_RGBA16) {
            const uint16_t *p = reinterpret_cast<const uint16_t *>(src) + (FORMAT == CE_PIXEL_RGB16 ? 3 : 4) * i;
            r = min((uint32_t)p[0], maxv), g = min((uint32_t)p[1], maxv), b = min((uint32_t)p[2], maxv);
        } else {
            const uint8_t *p = reinterpret_cast<const uint8_t *>(src) + (FORMAT == CE_PIXEL_RGB8 ? 3 : 4) * i;
            r = p[0], g = p[1], b = p[2];
        }
        dst[3 * i] = (uint16_t)r, dst[3 * i + 1] = (uint16_t)g, dst[3 * i + 2] = (uint16_t)b;
    }
}

// ---- ICC -> sRGB as a complete colour table (include/ce_metrics.h: ce_lut_*) ------------------------------------------
// the host's packed 3-byte table -> one dword per colour (r | g << 8 | b << 16), so a lookup is one aligned 4-byte gather
__global__ __launch_bounds__(256) void k_lut_expand(const uint8_t *__restrict__ packed, uint32_t *__restrict__ table, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        table[i] = (uint32_t)packed[3 * (size_t)i] | ((uint32_t)packed[3 * (size_t)i + 1] << 8) | ((uint32_t)packed[3 * (size_t)i + 2] << 16);
}

// in place on one packed RGB8 image of the slab: pixel -> table[(r << 16) | (g << 8) | b]
__global__ __launch_bounds__(256) void k_lut_apply(uint8_t *__restrict__ rgb, const uint32_t *__restrict__ table, size_t n_pixels)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x * blockDim.x) {
        uint8_t *p = rgb + 3 * i;
        const uint32_t v = table[((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[2]];
        p[0] = (uint8_t)v;
        p[1] = (uint8_t)(v >> 8);
        p[2] = (uint8_t)(v >> 16);
    }
}

}  // namespace

int ce_launch_lut_expand(ce_ctx *ctx, hipStream_t stream, const uint8_t *d_packed, uint32_t *d_table)
{
    CE_LAUNCH_ON(ctx, stream, "lut_expand", k_lut_expand, dim3(8192), dim3(256), 0, d_packed, d_table, 1u << 24);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

int ce_launch_lut_apply(ce_ctx *ctx, hipStream_t stream, uint8_t *d_rgb, const uint32_t *d_table, size_t n_pixels)
{
    if (n_pixels == 0) return CE_OK;
    const dim3 grid((uint32_t)std::min<size_t>((n_pixels + 255) / 256, 8192)), block(256);
    CE_LAUNCH_ON(ctx, stream, "lut_apply", k_lut_apply, grid, block, 0, d_rgb, d_table, n_pixels);
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

size_t ce_pixel_bytes(int format)
{
    switch (format) {
        case CE_PIXEL_RGB8: return 3;
        case CE_PIXEL_RGBA8: return 4;
        case CE_PIXEL_RGB16_10BIT: return 6;
        case CE_PIXEL_RGBA16_10BIT: return 8;
        case CE_PIXEL_RGB16: return 6;
        case CE_PIXEL_RGBA16: return 8;
        case CE_PIXEL_RGB_F32: return 12;
        default: return 0;
    }
}

int ce_launch_ingest(ce_ctx *ctx, hipStream_t stream, int format, const void *d_src, uint8_t *d_dst, size_t n_pixels)
{
    if (n_pixels == 0) return CE_OK;
    const dim3 grid((uint32_t)std::min<size_t>((n_pixels + 255) / 256, 8192)), block(256);
    switch (format) {
        case CE_PIXEL_RGBA8: CE_LAUNCH_ON(ctx, stream, "ingest_rgba8", k_ingest<CE_PIXEL_RGBA8>, grid, block, 0, d_src, d_dst, n_pixels); break;
        case CE_PIXEL_RGB16_10BIT:
            CE_LAUNCH_ON(ctx, stream, "ingest_rgb16", k_ingest<CE_PIXEL_RGB16_10BIT>, grid, block, 0, d_src, d_dst, n_pixels);
            break;
        case CE_PIXEL_RGBA16_10BIT:
            CE_LAUNCH_ON(ctx, stream, "ingest_rgba16", k_ingest<CE_PIXEL_RGBA16_10BIT>, grid, block, 0, d_src, d_dst, n_pixels);
            break;
        default: return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}

// d_src: 16-byte aligned (a hipMalloc'd staging image); d_dst: a slot of a deep slab
int ce_launch_ingest_deep(ce_ctx *ctx, hipStream_t stream, int format, uint32_t depth, const void *d_src, uint16_t *d_dst, size_t n_pixels)
{
    if (n_pixels == 0) return CE_OK;
    const uint32_t maxv = (1u << depth) - 1u;
    const dim3 grid((uint32_t)std::min<size_t>((n_pixels / 8 + 255) / 256 + 1, 8192)), block(256);
    switch (format) {
        case CE_PIXEL_RGB8: CE_LAUNCH_ON(ctx, stream, "ingest_deep_rgb8", k_ingest_deep<CE_PIXEL_RGB8>, grid, block, 0, d_src, d_dst, n_pixels, maxv); break;
        case CE_PIXEL_RGBA8: CE_LAUNCH_ON(ctx, stream, "ingest_deep_rgba8", k_ingest_deep<CE_PIXEL_RGBA8>, grid, block, 0, d_src, d_dst, n_pixels, maxv); break;
        case CE_PIXEL_RGB16: CE_LAUNCH_ON(ctx, stream, "ingest_deep_rgb16", k_ingest_deep<CE_PIXEL_RGB16>, grid, block, 0, d_src, d_dst, n_pixels, maxv); break;
        case CE_PIXEL_RGBA16: CE_LAUNCH_ON(ctx, stream, "ingest_deep_rgba16", k_ingest_deep<CE_PIXEL_RGBA16>, grid, block, 0, d_src, d_dst, n_pixels, maxv); break;
        default: return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
