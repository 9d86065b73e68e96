// The device code of the resampler (resample.hip) and the geometry of its launches, kept free of anything but the HIP
// keywords, min / max and blockIdx / threadIdx, so that tests/cpp/resample_kernel_host.cpp can compile the same text for the
// host - thread and block indices as loop variables, the LDS a heap block of the size the launch asks for - and run it
// under the host sanitizers against tables, sources and destinations allocated at exactly their size.  k_resample_h is
// split at its barrier for that: resample_h_stage fills the LDS, resample_h_body reads it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileBytes = kThreads * 4;         // row bytes a block covers (before the shift to dword alignment)
constexpr uint32_t kTilePixels = kTileBytes / 3 + 2;  // output pixels those bytes can touch
constexpr uint32_t kLdsInts = 12288;                  // 48 KiB of taps per block at most

// geometry of one pass: n_rows rows of out_row_bytes, image `img` of the destination at dst + img * dst_stride
struct pass_geom {
    const uint8_t *src;
    uint8_t *dst;
    size_t src_stride, dst_stride;  // bytes between images
    uint32_t src_row_bytes, out_row_bytes;
    uint32_t rows_per_img;  // output rows of an image
    uint32_t tiles;         // tiles per output row
};

// one pass as it is launched: `grid` blocks of kThreads; the horizontal pass stages its taps in lds_bytes of dynamic LDS
// (`lds`) or, when they do not fit, asks for none and reads the global table
struct pass_launch {
    pass_geom g;
    uint32_t grid;
    size_t lds_bytes;
    bool lds;
};

// a whole resample: the passes that run, in their order
struct resample_launch {
    bool horiz, vert;
    pass_launch h, v;
};

// n images of `rows` output rows: src_w -> dst_w pixels a row (horizontal, ksize taps a pixel) or rows of dst_w = src_w
// pixels (vertical, ksize 0); false when the launch would not fit its 32-bit indices
inline bool plan_pass(const uint8_t *src, size_t sstride, uint32_t src_w, uint8_t *dst, size_t dstride, uint32_t dst_w, uint32_t rows,
                      uint32_t n, uint32_t ksize, pass_launch *p)
{
    pass_geom *g = &p->g;
    g->src = src, g->dst = dst, g->src_stride = sstride, g->dst_stride = dstride;
    if ((uint64_t)src_w * 3 > 0x7fffffffull || (uint64_t)dst_w * 3 > 0x7fffffffull - 2 * kTileBytes) return false;
    g->src_row_bytes = src_w * 3, g->out_row_bytes = dst_w * 3;
    g->rows_per_img = rows;
    g->tiles = (g->out_row_bytes + 3 + kTileBytes - 1) / kTileBytes;  // + 3: the row may start at byte 3 of its first dword
    if ((uint64_t)g->tiles * rows * n > 0x7fffffffull) return false;
    p->grid = g->tiles * rows * n;
    const size_t lds = (size_t)(2 + ksize) * kTilePixels * sizeof(int32_t);
    p->lds = ksize != 0 && lds <= kLdsInts * sizeof(int32_t);
    p->lds_bytes = p->lds ? lds : 0;
    return true;
}

// n images of w x h, src_stride apart, to out_w x out_h, dst_stride apart.  horizontal: w -> out_w over the h source rows,
// into `mid` (n x h x out_w x 3 bytes) when a vertical pass follows; vertical: h -> out_h over rows of out_w pixels
inline bool plan_resample(const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, uint32_t w, uint32_t h, uint32_t out_w,
                          uint32_t out_h, uint32_t n, bool horiz, bool vert, uint32_t ksize_h, uint8_t *mid, resample_launch *r)
{
    const bool two = horiz && vert;
    const size_t mid_stride = (size_t)h * out_w * 3;
    r->horiz = horiz, r->vert = vert;
    if (horiz && !plan_pass(src, src_stride, w, two ? mid : dst, two ? mid_stride : dst_stride, out_w, h, n, ksize_h, &r->h)) return false;
    if (vert && !plan_pass(two ? mid : src, two ? mid_stride : src_stride, out_w, dst, dst_stride, out_w, out_h, n, 0, &r->v)) return false;
    return true;
}

__device__ __forceinline__ uint32_t clip8(uint32_t acc) { return (uint32_t)min(max((int32_t)acc >> 22, 0), 255); }

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
// Before the barrier: the block's taps into s_tab, LDS of [2 + ksize][kTilePixels] ints.
__device__ __forceinline__ void resample_h_stage(const place &p, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize,
                                                 int32_t *s_tab)
{
    const uint32_t x0 = (uint32_t)p.b0 / 3u;
    const uint32_t px = min(kTilePixels, n_out - x0);
    for (uint32_t i = threadIdx.x; i < px; i += kThreads) {
        s_tab[i] = tab[x0 + i];
        s_tab[kTilePixels + i] = tab[n_out + x0 + i];
    }
    for (uint32_t i = threadIdx.x; i < px * ksize; i += kThreads) {  // consecutive global words -> [tap][pixel]
        const uint32_t xl = i / ksize, t = i - xl * ksize;
        s_tab[(2 + t) * kTilePixels + xl] = tab[2 * (size_t)n_out + (size_t)x0 * ksize + i];
    }
}

// After it: the thread's dword of the output row.  LDS: taps from s_tab as resample_h_stage left them, else from `tab`
// (s_tab is not read).
template <bool LDS>
__device__ __forceinline__ void resample_h_body(const pass_geom &g, const place &p, const int32_t *__restrict__ tab, uint32_t n_out,
                                                uint32_t ksize, const int32_t *s_tab)
{
    const uint32_t x0 = (uint32_t)p.b0 / 3u;
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

__device__ __forceinline__ void resample_v_body(const pass_geom &g, const int32_t *__restrict__ tab, uint32_t n_out, uint32_t ksize)
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
