// The device code of the HLG ingest (codec-eval_amd/csrc/cicp_kernel.h's k_tagged and yuv_cicp_kernel.h's k_yuv_tagged with
// hlg_pixel.h's hlg_px as their pixel, and the yuv_kernel.h they build on) compiled for the host (hip_on_host.h): blockIdx /
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

#include "hip_on_host.h"
#include "ingest_host.h"

#include "cicp_kernel.h"
#include "hlg_pixel.h"
#include "yuv_cicp_kernel.h"
#include "yuv_ladder.h"

template <int FMT>
static void run_rgb(const hlg_args &a, bool matrix)
{
    const size_t blocks = std::max<size_t>((a.c.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_tagged's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_tagged<FMT>(hlg_px<true>{a}); else k_tagged<FMT>(hlg_px<false>{a});
        }
}

// one launch: every thread of every block of ce_launch_yuv_tagged's grid
static void run_yuv(int bps, int sub, bool semi, const yuv_args &y, const hlg_args &h, bool matrix)
{
    const size_t groups = (size_t)((y.w + 7) / 8) * ((y.h + 1) / 2), blocks = (groups + 63) / 64;
    yuv_ladder(bps == 1, sub, semi, [&](auto b, auto s, auto sm) {
        constexpr int BPS = decltype(b)::value, SUB = decltype(s)::value;
        constexpr bool SEMI = decltype(sm)::value;
        for (size_t blk = 0; blk < blocks; blk++)
            for (unsigned t = 0; t < 64; t++) {
                blockIdx.x = (unsigned)blk, threadIdx.x = t;
                if (matrix) k_yuv_tagged<BPS, SUB, SEMI>(yuv_px_args<hlg_px<true>>{y, {h}});
                else k_yuv_tagged<BPS, SUB, SEMI>(yuv_px_args<hlg_px<false>>{y, {h}});
            }
    });
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
    uint8_t *src = make_packed_source(src_bytes, format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16, maxv, seed);
    if (!src) return 67;
    if (zeros)
        for (size_t p = 0; p < (size_t)n_px; p++)
            if ((lcg_next(seed) >> 29) == 0) memset(src + p * bpp, 0, bpp);
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
    if (!front_guard_intact(slab, off, cases)) return 2;
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
    hlg_args a{};
    if (!read_pixel_args(in, a)) return 66;
    host_planes P;
    if (!make_planes(P, w, h, sub, semi, d, msb, pad, seed, out)) return 67;
    float *table = read_table(tf, table_offset, maxv);
    if (!table) return 69;
    const size_t slot_bytes = (size_t)w * h * 12, slab_bytes = (size_t)(slot + 2) * slot_bytes;
    uint8_t *slab = make_slab(slab_bytes, off);
    if (!slab) return 68;
    yuv_args y{};
    fill_yuv_args(y, P, w, h, d, msb, tri, k, (int64_t)maxv);
    a.c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), a.c.table = table, a.c.maxv = maxv;
    run_yuv(d == 8 ? 1 : 2, sub, semi != 0, y, a, has_matrix != 0);
    if (!front_guard_intact(slab, off, cases)) return 2;
    fwrite(slab + off, 1, slab_bytes, out);
    free(slab);
    free(table);
    free_planes(P);
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
