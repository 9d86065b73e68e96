// The resampler behind ce_resample_rgb8 / ce_batch_resample (include/ce_metrics.h): the two passes
// of a separable fixed-point convolution over packed RGB8, a horizontal pass over rows and a vertical pass over the
// image between them.  All arithmetic is integer - 22-bit weights built on the host (ce_tables.cpp), an int32
// accumulator, one arithmetic shift, a clip - so the output is a function of the tables and the input bytes alone.
//
// Both kernels are streams: a block covers kTileBytes consecutive bytes of ONE output row and a thread one dword of
// them, aligned in the destination slab (an image starts at any byte of its slab, a row at any byte of its image), so a
// wave's 64 stores are 256 consecutive bytes.  Only the first and the last dword of a tile can be partial; those are
// stored byte by byte.
//   horizontal  the taps differ from pixel to pixel: the block stages the tables of its <= kTilePixels output pixels in
//               LDS, tap-major ([tap][pixel]: a wave's lanes read consecutive words, the three bytes of a pixel the same
//               one), and falls back to the global table when a tile's taps exceed kLdsInts (scales beyond ~5)
//   vertical    every byte of an output row uses the same taps: they are indexed by the block alone, so the compiler
//               loads them through the scalar cache; a thread reads its four source bytes of a row as one (unaligned) word
#include "ce_internal.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileBytes = kThreads * 4;         // row bytes a block covers (before the shift to dword alignment)
constexpr uint32_t kTilePixels = kTileBytes / 3 + 2;  // output pixels those bytes can touch
constexpr uint32_t kLdsInts = 12288;                  // 48 KiB of taps per block at most

__device__ __forceinline__ uint32_t clip8(uint32_t acc) { return (uint32_t)min(max((int32_t)acc >> 22, 0), 255); }

// geometry of one pass: n_rows rows of out_row_bytes, image `img` of the destination at dst + img * dst_stride
struct pass_geom {
    const uint8_t *src;
    uint8_t *dst;
    size_t src_stride, dst_stride;  // bytes between images
    uint32_t src_row_bytes, out_row_bytes;
    uint32_t rows_per_img;  // output rows of an image
    uint32_t tiles;         // tiles per output row
};

// A block's place: its output row, the row-relative byte range [b0, b1) of its tile, and for this thread the row-relative
// byte `rb` (may be negative / beyond b1 at a tile's ends) of the dword it stores at `out`.
struct place {
    uint32_t img, y;
    int32_t b0, b1, rb;
    uint8_t *out;
};

__device__ __forceinline__ place find_place(const pass_geom &g)
{
    place p;
    const uint32_t row = blockIdx.x / g.tiles, tile = blockIdx.x - row * g.tiles;
    p.img = row / g.rows_per_img;
    p.y = row - p.img * g.rows_per_img;
    uint8_t *row_ptr = g.dst + (size_t)p.img * g.dst_stride + (size_t)p.y * g.out_row_bytes;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(row_ptr) & 3u);
    // tile t covers the dwords [t * kThreads, (t + 1) * kThreads) counted from the aligned word holding the row's first byte
    p.rb = (int32_t)((tile * kThreads + threadIdx.x) * 4u) - (int32_t)phase;
    p.b0 = max((int32_t)(tile * kTileBytes) - (int32_t)phase, 0);
    p.b1 = min((int32_t)((tile + 1) * kTileBytes) - (int32_t)phase, (int32_t)g.out_row_bytes);
    p.out = row_ptr + p.rb;
    return p;
}

__device__ __forceinline__ void store4(const place &p, const uint32_t v[4])
{
    if (p.rb >= p.b0 && p.rb + 4 <= p.b1) {
        *reinterpret_cast<uint32_t *>(p.out) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (p.rb + j >= p.b0 && p.rb + j < p.b1) p.out[j] = (uint8_t)v[j];
    }
}

// tab = [n_out] first tap | [n_out] tap count | [n_out][ksize] weights
template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_resample_h(pass_geom g, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    extern __shared__ int32_t s_tab[];  // LDS: [2 + ksize][kTilePixels]
    const place p = find_place(g);
    const uint32_t x0 = (uint32_t)p.b0 / 3u;
    if (LDS) {
        const uint32_t px = min(kTilePixels, n_out - x0);
        for (uint32_t i = threadIdx.x; i < px; i += kThreads) {
            s_tab[i] = tab[x0 + i];
            s_tab[kTilePixels + i] = tab[n_out + x0 + i];
        }
        for (uint32_t i = threadIdx.x; i < px * ksize; i += kThreads) {  // consecutive global words -> [tap][pixel]
            const uint32_t xl = i / ksize, t = i - xl * ksize;
            s_tab[(2 + t) * kTilePixels + xl] = tab[2 * (size_t)n_out + (size_t)x0 * ksize + i];
        }
        __syncthreads();
    }
    if (p.rb + 4 <= p.b0 || p.rb >= p.b1) return;
    const uint8_t *line = g.src + (size_t)p.img * g.src_stride + (size_t)p.y * g.src_row_bytes;
    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t b = p.rb + j;
        if (b < p.b0 || b >= p.b1) continue;
        const uint32_t x = (uint32_t)b / 3u, c = (uint32_t)b - x * 3u, xl = x - x0;
        const int32_t xmin = LDS ? s_tab[xl] : tab[x];
        const int32_t n = LDS ? s_tab[kTilePixels + xl] : tab[n_out + x];
        const uint8_t *s = line + (size_t)xmin * 3u + c;
        uint32_t acc = 1u << 21;
        for (int32_t t = 0; t < n; t++) {
            const int32_t k = LDS ? s_tab[(2 + t) * kTilePixels + xl] : tab[2 * (size_t)n_out + (size_t)x * ksize + t];
            acc += (uint32_t)k * s[(size_t)t * 3u];
        }
        v[j] = clip8(acc);
    }
    store4(p, v);
}

__global__ __launch_bounds__(kThreads) void k_resample_v(pass_geom g, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize)
{
    const place p = find_place(g);
    if (p.rb + 4 <= p.b0 || p.rb >= p.b1) return;
    // the row's taps: the same for every thread of the block
    const int32_t ymin = tab[p.y], n = tab[n_out + p.y];
    const int32_t *__restrict__ k = tab + 2 * (size_t)n_out + (size_t)p.y * ksize;
    const uint8_t *col = g.src + (size_t)p.img * g.src_stride + (size_t)ymin * g.src_row_bytes;
    uint32_t acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
    if (p.rb >= p.b0 && p.rb + 4 <= p.b1) {
        const uint8_t *s = col + p.rb;
        for (int32_t t = 0; t < n; t++, s += g.src_row_bytes) {
            uint32_t w;
            __builtin_memcpy(&w, s, 4);  // any alignment
            const uint32_t kt = (uint32_t)k[t];
            acc[0] += kt * (w & 255u);
            acc[1] += kt * ((w >> 8) & 255u);
            acc[2] += kt * ((w >> 16) & 255u);
            acc[3] += kt * (w >> 24);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (p.rb + j < p.b0 || p.rb + j >= p.b1) continue;
            const uint8_t *s = col + (p.rb + j);
            for (int32_t t = 0; t < n; t++, s += g.src_row_bytes) acc[j] += (uint32_t)k[t] * *s;
        }
    }
    const uint32_t v[4] = {clip8(acc[0]), clip8(acc[1]), clip8(acc[2]), clip8(acc[3])};
    store4(p, v);
}

}  // namespace

int ce_launch_resample(ce_ctx *ctx, hipStream_t stream, const uint8_t *d_src, size_t src_stride, uint8_t *d_dst, size_t dst_stride,
                       uint32_t w, uint32_t h, uint32_t out_w, uint32_t out_h, uint32_t n, const ce_resample_axis *horiz,
                       const ce_resample_axis *vert, uint8_t *mid)
{
    auto geom = [&](const uint8_t *src, size_t sstride, uint32_t src_w, uint8_t *dst, size_t dstride, uint32_t dst_w, uint32_t rows,
                    pass_geom *g) -> bool {
        g->src = src, g->dst = dst, g->src_stride = sstride, g->dst_stride = dstride;
        if ((uint64_t)src_w * 3 > 0x7fffffffull || (uint64_t)dst_w * 3 > 0x7fffffffull - 2 * kTileBytes) return false;
        g->src_row_bytes = src_w * 3, g->out_row_bytes = dst_w * 3;
        g->rows_per_img = rows;
        g->tiles = (g->out_row_bytes + 3 + kTileBytes - 1) / kTileBytes;  // + 3: the row may start at byte 3 of its first dword
        return (uint64_t)g->tiles * rows * n <= 0x7fffffffull;
    };
    pass_geom gh{}, gv{};
    const bool two = horiz && vert;
    // horizontal: w -> out_w over the h source rows, into `mid` when a vertical pass follows
    if (horiz && !geom(d_src, src_stride, w, two ? mid : d_dst, two ? (size_t)h * out_w * 3 : dst_stride, out_w, h, &gh)) goto too_large;
    // vertical: h -> out_h over rows of out_w pixels
    if (vert && !geom(two ? mid : d_src, two ? (size_t)h * out_w * 3 : src_stride, out_w, d_dst, dst_stride, out_w, out_h, &gv)) goto too_large;
    if (horiz) {
        const size_t lds = (size_t)(2 + horiz->ksize) * kTilePixels * sizeof(int32_t);
        const dim3 grid(gh.tiles * h * n);
        if (lds <= kLdsInts * sizeof(int32_t))
            CE_LAUNCH_ON(ctx, stream, "resample_h", k_resample_h<true>, grid, dim3(kThreads), lds, gh, horiz->d, out_w, horiz->ksize);
        else
            CE_LAUNCH_ON(ctx, stream, "resample_h_wide", k_resample_h<false>, grid, dim3(kThreads), 0, gh, horiz->d, out_w, horiz->ksize);
    }
    if (vert)
        CE_LAUNCH_ON(ctx, stream, "resample_v", k_resample_v, dim3(gv.tiles * out_h * n), dim3(kThreads), 0, gv, vert->d, out_h,
                     vert->ksize);
    {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->err = std::string("resample: ") + hipGetErrorString(e);
            return CE_ERR_BACKEND;
        }
    }
    return CE_OK;
too_large:
    ctx->err = "resample: too many tiles for one launch";
    return CE_ERR_INVALID_ARG;
}
