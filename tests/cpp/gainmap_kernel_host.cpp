// The device code of the gain-map ingest (codec-eval_amd/csrc/gainmap_kernel.h's k_gainmap with gainmap_pixel.h's pixel)
// compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain variables that a loop sets, and every thread of every
// block of a launch runs in turn.  Built with -ffp-contract=off -fsanitize=address,undefined by
// tests/test_gainmap_kernel_host_cpu.py: the base, the map, the transfer table, the log2-gain tables and the slab are
// allocated at exactly their size, the slab `off` bytes after a 16-byte boundary with a guard in front, so a load outside
// any of them or a store outside the slot stops the run, and so does a wide access to an address that is not a multiple of
// its width.
//
// usage: gainmap_kernel_host CONFIGS TABLES YTABLES OUT.  CONFIGS holds one case per line:
//   format w h gw gh channels slot off seed maxv table_offset ytable_offset has_matrix m[0] .. m[8] kb[0] .. kb[2] ka[0] .. ka[2]
// (the matrix as the bits of nine floats, the offsets per output channel as the bits of doubles).  TABLES is a file of
// floats; a case's transfer table is maxv + 1 of them from table_offset on.  YTABLES is a file of doubles; a case's
// log2-gain tables are 256 * channels of them from ytable_offset on.  The slab holds slot + 1 slots and a trailing guard slot,
// filled with 0xEE bytes; the image goes to slot `slot`.  OUT receives, per case, the base, the map, then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "gainmap_kernel.h"

template <int FMT, int NCH>
static void run_matrix(const gainmap_args &a, bool matrix)
{
    const size_t blocks = std::max<size_t>((a.c.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_gainmap's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_gainmap<FMT, NCH, true>(a); else k_gainmap<FMT, NCH, false>(a);
        }
}

template <int FMT>
static void run_format(const gainmap_args &a, int channels, bool matrix)
{
    if (channels == 3) run_matrix<FMT, 3>(a, matrix); else run_matrix<FMT, 1>(a, matrix);
}

static bool read_doubles(FILE *in, double *p, int n)
{
    for (int i = 0; i < n; i++) {
        unsigned long long bits;
        if (fscanf(in, "%llu", &bits) != 1) return false;
        memcpy(&p[i], &bits, 8);
    }
    return true;
}

static int one_case(FILE *in, FILE *tf, FILE *yf, FILE *out, int cases, int format)
{
    int off, has_matrix, channels;
    unsigned w, h, gw, gh, seed, maxv;
    unsigned long long slot, table_offset, ytable_offset;
    if (fscanf(in, "%u %u %u %u %d %llu %d %u %u %llu %llu %d", &w, &h, &gw, &gh, &channels, &slot, &off, &seed, &maxv, &table_offset, &ytable_offset,
               &has_matrix) != 12)
        return 66;
    gainmap_args a{};
    for (int i = 0; i < 9; i++) {
        uint32_t bits;
        if (fscanf(in, "%u", &bits) != 1) return 66;
        memcpy(&a.c.m[i], &bits, 4);
    }
    if (!read_doubles(in, a.kb, 3) || !read_doubles(in, a.ka, 3)) return 66;
    if ((channels != 1 && channels != 3) || gw < 1 || gw > w || gh < 1 || gh > h) return 72;
    const size_t n_px = (size_t)w * h, bpp = ce_pixel_bytes_of(format), src_bytes = n_px * bpp, slot_bytes = n_px * 12;
    if (bpp == 0) return 70;
    uint8_t *src = make_packed_source(src_bytes, format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16, maxv, seed);
    if (!src) return 67;
    fwrite(src, 1, src_bytes, out);
    const size_t map_bytes = (size_t)gw * gh * channels;
    uint8_t *map = static_cast<uint8_t *>(malloc(map_bytes));
    if (!map) return 67;
    fill_samples(map, map_bytes, seed);
    fwrite(map, 1, map_bytes, out);
    float *table = read_table(tf, table_offset, maxv);
    if (!table) return 69;
    const size_t n_y = (size_t)256 * channels;
    double *ytab = static_cast<double *>(malloc(n_y * 8));
    if (!ytab || fseek(yf, (long)(ytable_offset * 8), SEEK_SET) != 0 || fread(ytab, 8, n_y, yf) != n_y) return 69;
    const size_t slab_bytes = (size_t)(slot + 2) * slot_bytes;
    uint8_t *slab = make_slab(slab_bytes, off);
    if (!slab) return 68;
    a.c.src = src, a.c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), a.c.n_pixels = n_px, a.c.table = table, a.c.maxv = maxv;
    a.map = map, a.ytab = ytab, a.w = w, a.h = h, a.gw = gw, a.gh = gh;
    switch (format) {
        case CE_PIXEL_RGB8: run_format<CE_PIXEL_RGB8>(a, channels, has_matrix != 0); break;
        case CE_PIXEL_RGBA8: run_format<CE_PIXEL_RGBA8>(a, channels, has_matrix != 0); break;
        case CE_PIXEL_RGB16: run_format<CE_PIXEL_RGB16>(a, channels, has_matrix != 0); break;
        default: run_format<CE_PIXEL_RGBA16>(a, channels, has_matrix != 0); break;
    }
    if (!front_guard_intact(slab, off, cases)) return 2;
    fwrite(slab + off, 1, slab_bytes, out);
    free(slab);
    free(ytab);
    free(table);
    free(map);
    free(src);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *yf = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !tf || !yf || !out) return 65;
    int cases = 0, format;
    while (fscanf(in, "%d", &format) == 1) {
        if (const int rc = one_case(in, tf, yf, out, cases, format)) return rc;
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(yf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
