// The device code of the HLG ingest (codec-eval_amd/csrc/hlg_kernel.h and yuv_hlg_kernel.h, with the hlg_pixel.h, cicp_kernel.h,
// yuv_cicp_kernel.h and yuv_kernel.h they build on) compiled for the host: the HIP keywords are defined away, blockIdx /
// threadIdx are plain variables that a loop sets, and every thread of every block of a launch runs in turn.  Built with
// -ffp-contract=off -fsanitize=address,undefined by tests/test_hlg_kernel_host_cpu.py: the source (or each plane, at exactly
// the bytes its rows need), the table and the slab are allocated at exactly their size, the slab `off` bytes after a 16-byte
// boundary with a guard in front, so a load outside the source or the table or a store outside the slot stops the run, and
// so does a wide access to an address that is not a multiple of its width.
//
// usage: hlg_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line, by route:
//   rgb format n_pixels slot off seed zeros maxv table_offset has_matrix m[0] .. m[8] p[0] .. p[4]
//   yuv w h subsampling semiplanar triangle depth msb_aligned pad slot off seed KY KRV KGU KGV KBU y0 c0 maxv table_offset
//       has_matrix m[0] .. m[8] p[0] .. p[4]
// (the matrix as the bits of nine floats; p = kR, kG, kB, gamma - 1, A as the bits of five doubles; zeros: one pixel in
// eight is all zero, which gives ys == 0).  TABLES is a file of floats; a case's table is maxv + 1 of them from table_offset
// on.  The slab holds slot + 1 slots and a trailing guard slot, filled with 0xEE bytes; the image goes to slot `slot`.  OUT
// receives, per case, the source (rgb) or the planes' rows without padding (yuv: Y, then CbCr or Cb and Cr), then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct idx3 {
    unsigned x;
};
static idx3 blockIdx, threadIdx;
using std::max;
using std::min;
struct uint4 {
    uint32_t x, y, z, w;
};
struct uint2 {
    uint32_t x, y;
};
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
struct alignas(16) float4 {
    float x, y, z, w;
};
struct alignas(8) float2 {
    float x, y;
};
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
static inline float2 make_float2(float a, float b) { return {a, b}; }

#include "hlg_kernel.h"
#include "yuv_hlg_kernel.h"

static size_t ce_pixel_bytes_of(int format)  // ce_pixel_bytes of the four formats the ingest takes
{
    return format == CE_PIXEL_RGB8 ? 3 : format == CE_PIXEL_RGBA8 ? 4 : format == CE_PIXEL_RGB16 ? 6 : format == CE_PIXEL_RGBA16 ? 8 : 0;
}

template <int FMT>
static void run_rgb(const hlg_args &a, bool matrix)
{
    const size_t blocks = std::max<size_t>((a.c.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_hlg's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_hlg<FMT, true>(a); else k_hlg<FMT, false>(a);
        }
}

template <int BPS, int SUB, bool SEMI>
static void run(const yuv_hlg_args &a, bool matrix)
{
    const size_t groups = (size_t)((a.y.w + 7) / 8) * ((a.y.h + 1) / 2), blocks = (groups + 63) / 64;  // ce_launch_yuv_hlg's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < 64; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_yuv_hlg<BPS, SUB, SEMI, true>(a); else k_yuv_hlg<BPS, SUB, SEMI, false>(a);
        }
}
template <int BPS, int SUB>
static void run_layout(bool semi, const yuv_hlg_args &a, bool matrix)
{
    if (semi && SUB != CE_YUV_400) run<BPS, SUB, true>(a, matrix);
    else run<BPS, SUB, false>(a, matrix);
}
template <int BPS>
static void run_sub(int sub, bool semi, const yuv_hlg_args &a, bool matrix)
{
    switch (sub) {
        case CE_YUV_444: run_layout<BPS, CE_YUV_444>(semi, a, matrix); break;
        case CE_YUV_422: run_layout<BPS, CE_YUV_422>(semi, a, matrix); break;
        case CE_YUV_420: run_layout<BPS, CE_YUV_420>(semi, a, matrix); break;
        default: run_layout<BPS, CE_YUV_400>(semi, a, matrix); break;
    }
}

// the tail of a case's line: the matrix and the five doubles
static bool read_pixel_args(FILE *in, hlg_args &a)
{
    for (int i = 0; i < 9; i++) {
        uint32_t bits;
        if (fscanf(in, "%u", &bits) != 1) return false;
        memcpy(&a.c.m[i], &bits, 4);
    }
    double *p[5] = {&a.kr, &a.kg, &a.kb, &a.gm1, &a.a};
    for (int i = 0; i < 5; i++) {
        unsigned long long bits;
        if (fscanf(in, "%llu", &bits) != 1) return false;
        memcpy(p[i], &bits, 8);
    }
    return true;
}

static float *read_table(FILE *tf, unsigned long long table_offset, unsigned maxv)
{
    float *table = static_cast<float *>(malloc(((size_t)maxv + 1) * 4));
    if (!table || fseek(tf, (long)(table_offset * 4), SEEK_SET) != 0 || fread(table, 4, (size_t)maxv + 1, tf) != (size_t)maxv + 1) return nullptr;
    return table;
}

// the slab of slot + 2 slots behind `off` guard bytes, all 0xEE
static uint8_t *make_slab(size_t slab_bytes, int off)
{
    uint8_t *slab = static_cast<uint8_t *>(malloc(slab_bytes + (size_t)off));  // malloc: 16-byte aligned
    if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15)) return nullptr;
    memset(slab, 0xEE, slab_bytes + (size_t)off);
    return slab;
}

static int rgb_case(FILE *in, FILE *tf, FILE *out, int cases)
{
    int format, off, zeros, has_matrix;
    unsigned long long n_px, slot, table_offset;
    unsigned seed, maxv;
    if (fscanf(in, "%d %llu %llu %d %u %d %u %llu %d", &format, &n_px, &slot, &off, &seed, &zeros, &maxv, &table_offset, &has_matrix) != 9) return 66;
    hlg_args a{};
    if (!read_pixel_args(in, a)) return 66;
    const size_t bpp = ce_pixel_bytes_of(format), src_bytes = (size_t)n_px * bpp, slot_bytes = (size_t)n_px * 12;
    if (bpp == 0) return 70;
    auto next = [&seed] { return seed = seed * 1664525u + 1013904223u; };
    uint8_t *src = static_cast<uint8_t *>(malloc(src_bytes));
    if (!src || (reinterpret_cast<uintptr_t>(src) & 15)) return 67;  // malloc: 16-byte aligned, as the staging buffer is
    for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)(next() >> 24);
    if (format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16) {  // in range, but one sample in 16 above maxv
        for (size_t i = 0; i < src_bytes / 2; i++) {
            uint16_t v;
            memcpy(&v, src + 2 * i, 2);
            if ((next() >> 28) != 0) v &= (uint16_t)maxv;
            memcpy(src + 2 * i, &v, 2);
        }
    }
    if (zeros)
        for (size_t p = 0; p < (size_t)n_px; p++)
            if ((next() >> 29) == 0) memset(src + p * bpp, 0, bpp);
    fwrite(src, 1, src_bytes, out);
    float *table = read_table(tf, table_offset, maxv);
    if (!table) return 69;
    const size_t slab_bytes = (size_t)(slot + 2) * slot_bytes;
    uint8_t *slab = make_slab(slab_bytes, off);
    if (!slab) return 68;
    a.c.src = src, a.c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), a.c.n_pixels = (size_t)n_px, a.c.table = table, a.c.maxv = maxv;
    switch (format) {
        case CE_PIXEL_RGB8: run_rgb<CE_PIXEL_RGB8>(a, has_matrix != 0); break;
        case CE_PIXEL_RGBA8: run_rgb<CE_PIXEL_RGBA8>(a, has_matrix != 0); break;
        case CE_PIXEL_RGB16: run_rgb<CE_PIXEL_RGB16>(a, has_matrix != 0); break;
        default: run_rgb<CE_PIXEL_RGBA16>(a, has_matrix != 0); break;
    }
    for (int i = 0; i < off; i++)
        if (slab[i] != 0xEE) {
            fprintf(stderr, "case %d wrote in front of its slab\n", cases);
            return 2;
        }
    fwrite(slab + off, 1, slab_bytes, out);
    free(slab);
    free(table);
    free(src);
    return 0;
}

static int yuv_case(FILE *in, FILE *tf, FILE *out, int cases)
{
    int w, h, sub, semi, tri, d, msb, pad, off, has_matrix;
    unsigned long long slot, table_offset;
    unsigned seed, maxv;
    long long k[7];
    if (fscanf(in, "%d %d %d %d %d %d %d %d %llu %d %u %lld %lld %lld %lld %lld %lld %lld %u %llu %d", &w, &h, &sub, &semi, &tri, &d, &msb, &pad,
               &slot, &off, &seed, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5], &k[6], &maxv, &table_offset, &has_matrix) != 21)
        return 66;
    yuv_hlg_args a{};
    if (!read_pixel_args(in, a.h)) return 66;
    const int bps = d == 8 ? 1 : 2;
    const int cw = sub == CE_YUV_444 ? w : (w + 1) / 2, ch = sub == CE_YUV_420 ? (h + 1) / 2 : h;
    const int n_planes = sub == CE_YUV_400 ? 1 : semi ? 2 : 3;
    const size_t rows[3] = {(size_t)h, (size_t)ch, (size_t)ch};
    const size_t row_bytes[3] = {(size_t)w * bps, (size_t)(semi ? 2 * cw : cw) * bps, (size_t)cw * bps};
    uint8_t *plane[3] = {};
    size_t pitch[3] = {};
    auto next = [&seed] { return seed = seed * 1664525u + 1013904223u; };
    for (int p = 0; p < n_planes; p++) {
        pitch[p] = row_bytes[p] + (size_t)pad;
        const size_t size = (rows[p] - 1) * pitch[p] + row_bytes[p];  // what a caller owns, to the byte
        plane[p] = static_cast<uint8_t *>(malloc(size));
        if (!plane[p]) return 67;
        for (size_t i = 0; i < size; i++) plane[p][i] = (uint8_t)(next() >> 24);
        if (bps == 2 && !msb)  // low-aligned: in range, but one sample in 16 above it (ingest clamps those)
            for (size_t r = 0; r < rows[p]; r++)
                for (size_t i = 0; i < row_bytes[p] / 2; i++) {
                    uint16_t v;
                    memcpy(&v, plane[p] + r * pitch[p] + 2 * i, 2);
                    if ((next() >> 28) != 0) v &= (uint16_t)((1u << d) - 1u);
                    memcpy(plane[p] + r * pitch[p] + 2 * i, &v, 2);
                }
        for (size_t r = 0; r < rows[p]; r++) fwrite(plane[p] + r * pitch[p], 1, row_bytes[p], out);
    }
    float *table = read_table(tf, table_offset, maxv);
    if (!table) return 69;
    const size_t slot_bytes = (size_t)w * h * 12, slab_bytes = (size_t)(slot + 2) * slot_bytes;
    uint8_t *slab = make_slab(slab_bytes, off);
    if (!slab) return 68;
    yuv_args &y = a.y;
    y.p0 = plane[0], y.p1 = plane[1], y.p2 = plane[2];
    y.pitch0 = pitch[0], y.pitch1 = pitch[1], y.pitch2 = pitch[2];
    y.w = (uint32_t)w, y.h = (uint32_t)h, y.cw = (uint32_t)cw, y.ch = (uint32_t)ch;
    y.shift = msb ? 16u - (uint32_t)d : 0u, y.maxv = (1u << d) - 1u, y.triangle = tri;
    y.ky = k[0], y.krv = k[1], y.kgu = k[2], y.kgv = k[3], y.kbu = k[4], y.y0 = k[5], y.c0 = k[6];
    y.m = (int64_t)maxv;
    a.h.c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), a.h.c.table = table, a.h.c.maxv = maxv;
    if (bps == 1) run_sub<1>(sub, semi != 0, a, has_matrix != 0);
    else run_sub<2>(sub, semi != 0, a, has_matrix != 0);
    for (int i = 0; i < off; i++)
        if (slab[i] != 0xEE) {
            fprintf(stderr, "case %d wrote in front of its slab\n", cases);
            return 2;
        }
    fwrite(slab + off, 1, slab_bytes, out);
    free(slab);
    free(table);
    for (int p = 0; p < n_planes; p++) free(plane[p]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    char route[8];
    int cases = 0;
    while (fscanf(in, "%7s", route) == 1) {
        const int rc = strcmp(route, "rgb") == 0 ? rgb_case(in, tf, out, cases) : strcmp(route, "yuv") == 0 ? yuv_case(in, tf, out, cases) : 71;
        if (rc) return rc;
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
