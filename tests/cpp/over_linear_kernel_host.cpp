// The device code of linear-light compositing (codec-eval_amd/csrc/over_linear_kernel.h: k_tagged_over with cicp_pixel.h's
// cicp_px as its pixel, and k_linear_over) compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain variables that
// a loop sets, and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off
// -fsanitize=address,undefined by tests/test_over_linear_kernel_host_cpu.py: the source, the two tables and the slab are
// allocated at exactly their size - the slab ends with the last slot the launch writes, `off` bytes after a 16-byte boundary
// with a guard in front - so a load outside the source or a table or a store outside the slots stops the run, and so does a
// wide access to an address that is not a multiple of its width.
//
// usage: over_linear_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line:
//   format n_pixels first off seed maxv table_offset atab_offset has_matrix premul n_bg m[0] .. m[8] bg[0] .. bg[3 * n_bg - 1]
// (the matrix and the backgrounds as the bits of floats).  format: CE_PIXEL_RGBA8 / RGBA16, or CE_PIXEL_RGBA_F32 (maxv, the
// tables and the matrix unused).  TABLES is a file of floats; a case's transfer table is maxv + 1 of them from table_offset
// on, its alpha table maxv + 1 from atab_offset on.  The slab holds first + n_bg slots, all 0xEE before the launch; the image
// goes to slots first .. first + n_bg - 1.  OUT receives, per case, the source and then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "over_linear_kernel.h"

static size_t grid_of(size_t n_pixels) { return std::max<size_t>((n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1); }  // the launchers' grid

template <int FMT>
static void run(const cicp_args &a, bool matrix, const over_args &o)
{
    for (size_t b = 0; b < grid_of(a.n_pixels); b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_tagged_over<FMT>(cicp_px<true>{a}, o); else k_tagged_over<FMT>(cicp_px<false>{a}, o);
        }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    int format, off, has_matrix, premul;
    unsigned long long n_px, first, table_offset, atab_offset;
    unsigned seed, maxv, n_bg;
    int cases = 0;
    while (fscanf(in, "%d %llu %llu %d %u %u %llu %llu %d %d %u", &format, &n_px, &first, &off, &seed, &maxv, &table_offset, &atab_offset, &has_matrix,
                  &premul, &n_bg) == 11) {
        cicp_args a{};
        over_args o{};
        if (n_bg == 0 || n_bg > CE_MAX_BACKGROUNDS) return 71;
        for (int i = 0; i < 9; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&a.m[i], &bits, 4);
        }
        for (unsigned i = 0; i < 3 * n_bg; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&o.bg[i / 3][i % 3], &bits, 4);
        }
        const bool f32 = format == CE_PIXEL_RGBA_F32, wide = format == CE_PIXEL_RGBA16;
        if (!f32 && !wide && format != CE_PIXEL_RGBA8) return 70;
        const size_t bpp = f32 ? 16 : wide ? 8 : 4, src_bytes = (size_t)n_px * bpp, slot_bytes = (size_t)n_px * 12;
        auto next = [&seed] { return lcg_next(seed); };
        uint8_t *src = make_packed_source(src_bytes, wide, maxv, seed);
        if (!src) return 67;
        if (f32) {  // plausible values, with NaN, infinities, huge values and arbitrary bits sprinkled in; alphas around [0, 1]
            for (size_t i = 0; i < src_bytes / 4; i++) {
                const unsigned sel = next() >> 28;
                float v = (float)(int32_t)(next() >> 8) / 4194304.0f - 1.0f;  // [-1, 3)
                if (i % 4 == 3) v = (float)(next() >> 8) / 16777216.0f;       // alpha: [0, 1)
                uint32_t bits;
                if (sel == 0) bits = 0x7fc00000u | (next() & 0xffffu), memcpy(&v, &bits, 4);
                if (sel == 1) bits = (next() & 1u) ? 0x7f800000u : 0xff800000u, memcpy(&v, &bits, 4);
                if (sel == 2) v = (next() & 1u) ? 1e9f : -1e9f;
                if (sel == 3) memcpy(&v, src + 4 * i, 4);  // arbitrary bits
                if (i % 4 == 3 && sel >= 4 && sel < 8) v = sel == 4 ? 0.0f : sel == 5 ? 1.0f : sel == 6 ? -0.0f : 1.5f;
                memcpy(src + 4 * i, &v, 4);
            }
        } else {  // half of the alphas are 0, 1, maxv - 1, maxv or above maxv; the rest stay the generator's
            for (size_t p = 0; p < (size_t)n_px; p++) {
                const unsigned sel = next() >> 28;
                if (sel >= 8) continue;
                const unsigned above = wide && maxv < 0xffffu ? maxv + 1u + (next() % (0xffffu - maxv)) : maxv;
                const unsigned v = sel < 2 ? 0u : sel < 4 ? maxv : sel == 4 ? 1u : sel == 5 ? maxv - 1u : above;
                if (wide) {
                    const uint16_t s = (uint16_t)v;
                    memcpy(src + p * 8 + 6, &s, 2);
                } else {
                    src[p * 4 + 3] = (uint8_t)v;
                }
            }
        }
        fwrite(src, 1, src_bytes, out);
        float *table = nullptr, *atab = nullptr;
        if (!f32) {
            table = read_table(tf, table_offset, maxv);
            atab = read_table(tf, atab_offset, maxv);
            if (!table || !atab) return 69;
        }
        const size_t slab_bytes = (size_t)(first + n_bg) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        float *dst = reinterpret_cast<float *>(slab + off + (size_t)first * slot_bytes);
        o.atab = atab, o.n_bg = n_bg, o.slot_floats = (size_t)n_px * 3;
        if (f32) {
            for (size_t b = 0; b < grid_of((size_t)n_px); b++)
                for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
                    blockIdx.x = (unsigned)b, threadIdx.x = t;
                    if (premul) k_linear_over<true>(reinterpret_cast<const float *>(src), dst, (size_t)n_px, o);
                    else k_linear_over<false>(reinterpret_cast<const float *>(src), dst, (size_t)n_px, o);
                }
        } else {
            a.src = src, a.dst = dst, a.n_pixels = (size_t)n_px, a.table = table, a.maxv = maxv;
            if (wide) run<CE_PIXEL_RGBA16>(a, has_matrix != 0, o); else run<CE_PIXEL_RGBA8>(a, has_matrix != 0, o);
        }
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        free(atab);
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
