// What the ingest harnesses (cicp_kernel_host.cpp, yuv_cicp_kernel_host.cpp, hlg_kernel_host.cpp and, for the planes,
// yuv_kernel_host.cpp) build a case from: the source filled by the case's LCG, planes and a table allocated at exactly their
// size, and the slab behind its front guard.  Every block is a malloc of its own, so AddressSanitizer sees an access one byte
// outside it.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ce_metrics.h"

static inline size_t ce_pixel_bytes_of(int format)  // ce_pixel_bytes of the four formats the tagged ingest takes; 0: another
{
    return format == CE_PIXEL_RGB8 ? 3 : format == CE_PIXEL_RGBA8 ? 4 : format == CE_PIXEL_RGB16 ? 6 : format == CE_PIXEL_RGBA16 ? 8 : 0;
}

// the generator of every case's source: seed is the case's and moves on
static inline unsigned lcg_next(unsigned &seed) { return seed = seed * 1664525u + 1013904223u; }

// n bytes of the LCG's
static inline void fill_samples(uint8_t *p, size_t n, unsigned &seed)
{
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(lcg_next(seed) >> 24);
}
// u16 samples that are not MSB-aligned: in range, except one sample in 16, which stays above maxv (the ingest clamps those)
static inline void mask_u16(uint8_t *p, size_t n_samples, unsigned maxv, unsigned &seed)
{
    for (size_t i = 0; i < n_samples; i++) {
        uint16_t v;
        memcpy(&v, p + 2 * i, 2);
        if ((lcg_next(seed) >> 28) != 0) v &= (uint16_t)maxv;
        memcpy(p + 2 * i, &v, 2);
    }
}

// a packed source of src_bytes at malloc's 16-byte alignment, as the staging buffer is; nullptr: exit code 67
static inline uint8_t *make_packed_source(size_t src_bytes, bool u16, unsigned maxv, unsigned &seed)
{
    uint8_t *src = static_cast<uint8_t *>(malloc(src_bytes));
    if (!src || (reinterpret_cast<uintptr_t>(src) & 15)) return nullptr;
    fill_samples(src, src_bytes, seed);
    if (u16) mask_u16(src, src_bytes / 2, maxv, seed);
    return src;
}

// maxv + 1 floats from table_offset floats into tf; nullptr: exit code 69
static inline float *read_table(FILE *tf, unsigned long long table_offset, unsigned maxv)
{
    float *table = static_cast<float *>(malloc(((size_t)maxv + 1) * 4));
    if (!table || fseek(tf, (long)(table_offset * 4), SEEK_SET) != 0 || fread(table, 4, (size_t)maxv + 1, tf) != (size_t)maxv + 1) return nullptr;
    return table;
}

// slab_bytes behind `off` guard bytes, all 0xEE, from malloc's 16-byte boundary; nullptr: exit code 68
static inline uint8_t *make_slab(size_t slab_bytes, int off)
{
    uint8_t *slab = static_cast<uint8_t *>(malloc(slab_bytes + (size_t)off));
    if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15)) return nullptr;
    memset(slab, 0xEE, slab_bytes + (size_t)off);
    return slab;
}
// false (exit code 2) and a line on stderr if the guard bytes in front changed
static inline bool front_guard_intact(const uint8_t *slab, int off, int case_index)
{
    for (int i = 0; i < off; i++)
        if (slab[i] != 0xEE) {
            fprintf(stderr, "case %d wrote in front of its slab\n", case_index);
            return false;
        }
    return true;
}

// The planes of one w x h Y'CbCr image: each allocated at exactly the bytes its rows need ((rows - 1) * pitch + row bytes,
// what a caller owns, to the byte), filled by the LCG and written to `out` row by row without the padding
struct host_planes {
    int n_planes, cw, ch;
    uint8_t *plane[3];
    size_t pitch[3];
};
static inline bool make_planes(host_planes &P, int w, int h, int sub, int semi, int d, int msb, int pad, unsigned &seed, FILE *out)  // false: exit code 67
{
    const int bps = d == 8 ? 1 : 2;
    P = host_planes{};
    P.cw = sub == CE_YUV_444 ? w : (w + 1) / 2, P.ch = sub == CE_YUV_420 ? (h + 1) / 2 : h;
    P.n_planes = sub == CE_YUV_400 ? 1 : semi ? 2 : 3;
    const size_t rows[3] = {(size_t)h, (size_t)P.ch, (size_t)P.ch};
    const size_t row_bytes[3] = {(size_t)w * bps, (size_t)(semi ? 2 * P.cw : P.cw) * bps, (size_t)P.cw * bps};
    for (int p = 0; p < P.n_planes; p++) {
        P.pitch[p] = row_bytes[p] + (size_t)pad;
        const size_t size = (rows[p] - 1) * P.pitch[p] + row_bytes[p];
        P.plane[p] = static_cast<uint8_t *>(malloc(size));
        if (!P.plane[p]) return false;
        fill_samples(P.plane[p], size, seed);
        if (bps == 2 && !msb)
            for (size_t r = 0; r < rows[p]; r++) mask_u16(P.plane[p] + r * P.pitch[p], row_bytes[p] / 2, (1u << d) - 1u, seed);
        for (size_t r = 0; r < rows[p]; r++) fwrite(P.plane[p] + r * P.pitch[p], 1, row_bytes[p], out);
    }
    return true;
}
static inline void free_planes(host_planes &P)
{
    for (int p = 0; p < P.n_planes; p++) free(P.plane[p]);
}

// yuv_kernel.h's yuv_args of those planes, as ce_fill_yuv_args fills them: k = ce_yuv_coefficients' seven, m the output's maximum
template <class YuvArgs>
static inline void fill_yuv_args(YuvArgs &y, const host_planes &P, int w, int h, int d, int msb, int tri, const long long (&k)[7], int64_t m)
{
    y.p0 = P.plane[0], y.p1 = P.plane[1], y.p2 = P.plane[2];
    y.pitch0 = P.pitch[0], y.pitch1 = P.pitch[1], y.pitch2 = P.pitch[2];
    y.w = (uint32_t)w, y.h = (uint32_t)h, y.cw = (uint32_t)P.cw, y.ch = (uint32_t)P.ch;
    y.shift = msb ? 16u - (uint32_t)d : 0u, y.maxv = (1u << d) - 1u, y.triangle = tri;
    y.ky = k[0], y.krv = k[1], y.kgu = k[2], y.kgv = k[3], y.kbu = k[4], y.y0 = k[5], y.c0 = k[6];
    y.m = m;
}
