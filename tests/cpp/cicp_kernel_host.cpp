// The device code of the CICP ingest (codec-eval_amd/csrc/cicp_kernel.h's k_tagged with cicp_pixel.h's cicp_px as its pixel)
// and of the linear-f32 upload compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain variables that a loop
// sets, and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off -fsanitize=address,undefined by
// tests/test_cicp_kernel_host_cpu.py: the source, the table and the slab are allocated at exactly their size, the slab `off`
// bytes after a 16-byte boundary with a guard in front, so a load outside the source or the table or a store outside the
// slot stops the run, and so does a wide access to an address that is not a multiple of its width.
//
// usage: cicp_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line:
//   format n_pixels slot off seed maxv table_offset has_matrix m[0] .. m[8]   (the matrix as the bits of nine floats)
// format: the CE_PIXEL_* value, or CE_PIXEL_RGB_F32 for the f32 upload (n_pixels * 3 floats; maxv, table and matrix unused).  TABLES is a
// file of floats; a case's table is maxv + 1 of them from table_offset on.  The slab holds slot + 1 slots and a trailing
// guard slot filled with 0xEE bytes; the image goes to slot `slot`.  OUT receives, per case, the source and then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "cicp_kernel.h"

template <int FMT>
static void run(const cicp_args &a, bool matrix)
{
    const size_t blocks = std::max<size_t>((a.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_tagged's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_tagged<FMT>(cicp_px<true>{a}); else k_tagged<FMT>(cicp_px<false>{a});
        }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    int format, off, has_matrix;
    unsigned long long n_px, slot, table_offset;
    unsigned seed, maxv;
    int cases = 0;
    while (fscanf(in, "%d %llu %llu %d %u %u %llu %d", &format, &n_px, &slot, &off, &seed, &maxv, &table_offset, &has_matrix) == 8) {
        cicp_args a{};
        for (int i = 0; i < 9; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&a.m[i], &bits, 4);
        }
        const bool f32 = format == CE_PIXEL_RGB_F32;
        const size_t bpp = f32 ? 12 : ce_pixel_bytes_of(format), src_bytes = (size_t)n_px * bpp, slot_bytes = (size_t)n_px * 12;
        if (bpp == 0) return 70;
        auto next = [&seed] { return lcg_next(seed); };
        uint8_t *src = make_packed_source(src_bytes, format == CE_PIXEL_RGB16 || format == CE_PIXEL_RGBA16, maxv, seed);
        if (!src) return 67;
        if (f32) {  // plausible values, with NaN, infinities and huge values sprinkled in
            for (size_t i = 0; i < src_bytes / 4; i++) {
                const unsigned sel = next() >> 28;
                float v = (float)(int32_t)(next() >> 8) / 4194304.0f - 1.0f;  // [-1, 3)
                uint32_t bits;
                if (sel == 0) bits = 0x7fc00000u | (next() & 0xffffu), memcpy(&v, &bits, 4);
                if (sel == 1) bits = (next() & 1u) ? 0x7f800000u : 0xff800000u, memcpy(&v, &bits, 4);
                if (sel == 2) v = (next() & 1u) ? 1e9f : -1e9f;
                if (sel == 3) memcpy(&v, src + 4 * i, 4);  // arbitrary bits
                memcpy(src + 4 * i, &v, 4);
            }
        }
        fwrite(src, 1, src_bytes, out);
        float *table = nullptr;
        if (!f32) {
            table = read_table(tf, table_offset, maxv);
            if (!table) return 69;
        }
        const size_t slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        float *dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes);
        if (f32) {
            const size_t n = (size_t)n_px * 3, blocks = std::max<size_t>((n / 4 + kCicpBlock - 1) / kCicpBlock, 1);
            for (size_t b = 0; b < blocks; b++)
                for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
                    blockIdx.x = (unsigned)b, threadIdx.x = t;
                    k_linear_sanitise(reinterpret_cast<const float *>(src), dst, n);
                }
        } else {
            a.src = src, a.dst = dst, a.n_pixels = (size_t)n_px, a.table = table, a.maxv = maxv;
            switch (format) {
                case CE_PIXEL_RGB8: run<CE_PIXEL_RGB8>(a, has_matrix != 0); break;
                case CE_PIXEL_RGBA8: run<CE_PIXEL_RGBA8>(a, has_matrix != 0); break;
                case CE_PIXEL_RGB16: run<CE_PIXEL_RGB16>(a, has_matrix != 0); break;
                default: run<CE_PIXEL_RGBA16>(a, has_matrix != 0); break;
            }
        }
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        free(table);
        free(src);
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
