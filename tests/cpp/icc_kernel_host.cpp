// The device code of the ICC ingest (codec-eval_amd/csrc/icc_kernel.h's k_icc_encode and cicp_kernel.h's k_tagged, each with
// icc_pixel.h's icc_px as its pixel) compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain variables that a
// loop sets, and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off
// -fsanitize=address,undefined by tests/test_icc_kernel_host_cpu.py: the source, each channel's table, the thresholds and the
// slab are allocated at exactly their size - the thresholds with their entry 0, which the search must not read, poisoned -
// and the slab `off` bytes after a 16-byte boundary with a guard in front, so a load outside a buffer or a store outside the
// slot stops the run, and so does a wide access to an address that is not a multiple of its width.
//
// usage: icc_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line:
//   format n_pixels slot off seed maxv table_offset has_matrix out_kind depth_out thr_offset m[0] .. m[8]
// (the matrix as the bits of nine floats).  out_kind: 0 packed f32, 1 packed u8, 2 packed u16.  TABLES is a file of floats: a
// case's tone tables are 3 x (maxv + 1) of them from table_offset on, its thresholds T[1 .. 2^depth_out - 1] from thr_offset
// on.  The slab holds slot + 1 slots and a trailing guard slot filled with 0xEE bytes; the image goes to slot `slot`.  OUT
// receives, per case, the source and then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <sanitizer/asan_interface.h>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "icc_kernel.h"

template <int FMT, bool MATRIX>
static void run_px(const icc_args &a, int out_kind, void *dst, const float *thr, uint32_t top)
{
    const size_t blocks = std::max<size_t>((a.c.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_icc's grid
    const icc_px<MATRIX> px{a};
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (out_kind == 0) k_tagged<FMT>(px);
            else if (out_kind == 1) k_icc_encode<FMT, false>(px, dst, thr, top);
            else k_icc_encode<FMT, true>(px, dst, thr, top);
        }
}

template <int FMT>
static void run(const icc_args &a, bool matrix, int out_kind, void *dst, const float *thr, uint32_t top)
{
    if (matrix) run_px<FMT, true>(a, out_kind, dst, thr, top); else run_px<FMT, false>(a, out_kind, dst, thr, top);
}

// n floats from `offset` floats into tf, in an allocation of exactly n floats
static float *read_floats(FILE *tf, unsigned long long offset, size_t n)
{
    float *p = static_cast<float *>(malloc(n * 4));
    if (!p || fseek(tf, (long)(offset * 4), SEEK_SET) != 0 || fread(p, 4, n, tf) != n) return nullptr;
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    int format, off, has_matrix, out_kind;
    unsigned long long n_px, slot, table_offset, thr_offset;
    unsigned seed, maxv, depth_out;
    int cases = 0;
    while (fscanf(in, "%d %llu %llu %d %u %u %llu %d %d %u %llu", &format, &n_px, &slot, &off, &seed, &maxv, &table_offset, &has_matrix, &out_kind,
                  &depth_out, &thr_offset) == 11) {
        icc_args a{};
        for (int i = 0; i < 9; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&a.c.m[i], &bits, 4);
        }
        const size_t bpp = ce_pixel_bytes_of(format), src_bytes = (size_t)n_px * bpp;
        const size_t slot_bytes = (size_t)n_px * 3 * (out_kind == 0 ? 4 : out_kind == 1 ? 1 : 2);
        if (bpp == 0 || out_kind < 0 || out_kind > 2) return 70;
        uint8_t *src = make_packed_source(src_bytes, format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16, maxv, seed);
        if (!src) return 67;
        fwrite(src, 1, src_bytes, out);
        float *table[3];
        for (int c = 0; c < 3; c++) {
            table[c] = read_floats(tf, table_offset + (unsigned long long)c * (maxv + 1ull), (size_t)maxv + 1);
            if (!table[c]) return 69;
        }
        // thr[k] = T[k] for k = 1 .. 2^depth_out - 1 sits one float into its allocation, so that entry 0 ends an 8-byte
        // granule of the allocator's and that granule can be poisoned whole: a read of entry 0 stops the run
        float *thr_block = nullptr;
        const size_t n_thr = ((size_t)1 << depth_out) - 1;
        if (out_kind != 0) {
            thr_block = static_cast<float *>(malloc((n_thr + 2) * 4));
            if (!thr_block || (reinterpret_cast<uintptr_t>(thr_block) & 7) || fseek(tf, (long)(thr_offset * 4), SEEK_SET) != 0 ||
                fread(thr_block + 2, 4, n_thr, tf) != n_thr)
                return 69;
            ASAN_POISON_MEMORY_REGION(thr_block, 8);
        }
        const size_t slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        void *dst = slab + off + (size_t)slot * slot_bytes;
        a.c.src = src, a.c.dst = out_kind == 0 ? static_cast<float *>(dst) : nullptr, a.c.n_pixels = (size_t)n_px, a.c.maxv = maxv;
        a.c.table = table[0], a.table_g = table[1], a.table_b = table[2];
        const float *thr1 = thr_block ? thr_block + 1 : nullptr;
        const uint32_t top = out_kind != 0 ? 1u << (depth_out - 1) : 0u;
        switch (format) {
            case CE_PIXEL_RGB8: run<CE_PIXEL_RGB8>(a, has_matrix != 0, out_kind, dst, thr1, top); break;
            case CE_PIXEL_RGBA8: run<CE_PIXEL_RGBA8>(a, has_matrix != 0, out_kind, dst, thr1, top); break;
            case CE_PIXEL_RGB16: run<CE_PIXEL_RGB16>(a, has_matrix != 0, out_kind, dst, thr1, top); break;
            default: run<CE_PIXEL_RGBA16>(a, has_matrix != 0, out_kind, dst, thr1, top); break;
        }
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        if (thr_block) ASAN_UNPOISON_MEMORY_REGION(thr_block, 8);
        free(thr_block);
        for (int c = 0; c < 3; c++) free(table[c]);
        free(src);
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
