// The device code of the LUT-based ICC ingest (codec-eval_amd/csrc/icc_kernel.h's k_icc_encode and cicp_kernel.h's k_tagged,
// each with icc_lut_pixel.h's icc_lut_px as its pixel) compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain
// variables that a loop sets, and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off
// -fsanitize=address,undefined by tests/test_icc_lut_kernel_host_cpu.py: the source, each channel's input table, the CLUT, each
// sampled curve, the thresholds and the slab are allocated at exactly their size, the slab `off` bytes after a 16-byte
// boundary with a guard in front, so a load outside a buffer or a store outside the slot stops the run, and so does a wide
// access to an address that is not a multiple of its width.
//
// usage: icc_lut_kernel_host CONFIGS TABLES SOURCES OUT.  CONFIGS holds one case per line:
//   format n_pixels slot off src_offset maxv table_offset out_kind depth_out thr_offset tetra clut_offset g0 g1 g2 pcs has_matrix
//   mat_offset pcs_matrix_offset, then for each of the six curves: kind n sample_offset q[0] .. q[6] (the bits of seven doubles)
// out_kind: 0 packed f32, 1 packed u8, 2 packed u16.  TABLES is a file of floats that the offsets count in; g0 = 0: no CLUT.
// SOURCES is a file of bytes: a case's source is n_pixels pixels from src_offset on.  The slab holds slot + 1 slots and a
// trailing guard slot filled with 0xEE bytes; the image goes to slot `slot`.  OUT receives, per case, the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "icc_kernel.h"
#include "icc_lut_pixel.h"

template <int FMT, bool TETRA>
static void run_px(const icc_lut_args &a, int out_kind, void *dst, const float *thr, uint32_t top)
{
    const size_t blocks = std::max<size_t>((a.c.n_pixels / 4 + kCicpBlock - 1) / kCicpBlock, 1);  // ce_launch_icc_lut's grid
    const icc_lut_px<TETRA> px{a};
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kCicpBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (out_kind == 0) k_tagged<FMT>(px);
            else if (out_kind == 1) k_icc_encode<FMT, false>(px, dst, thr, top);
            else k_icc_encode<FMT, true>(px, dst, thr, top);
        }
}

template <int FMT>
static void run(const icc_lut_args &a, bool tetra, int out_kind, void *dst, const float *thr, uint32_t top)
{
    if (tetra) run_px<FMT, true>(a, out_kind, dst, thr, top); else run_px<FMT, false>(a, out_kind, dst, thr, top);
}

// n floats from `offset` floats into tf, in an allocation of exactly n floats (16-byte aligned, as hipMalloc's are)
static float *read_floats(FILE *tf, unsigned long long offset, size_t n)
{
    float *p = static_cast<float *>(malloc(n * 4));
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15) || fseek(tf, (long)(offset * 4), SEEK_SET) != 0 || fread(p, 4, n, tf) != n) return nullptr;
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *sf = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !tf || !sf || !out) return 65;
    int format, off, out_kind, tetra, has_matrix;
    unsigned long long n_px, slot, src_offset, table_offset, thr_offset, clut_offset, mat_offset, pcsm_offset;
    unsigned maxv, depth_out, g[3], pcs;
    int cases = 0;
    while (fscanf(in, "%d %llu %llu %d %llu %u %llu %d %u %llu %d %llu %u %u %u %u %d %llu %llu", &format, &n_px, &slot, &off, &src_offset, &maxv, &table_offset,
                  &out_kind, &depth_out, &thr_offset, &tetra, &clut_offset, &g[0], &g[1], &g[2], &pcs, &has_matrix, &mat_offset, &pcsm_offset) == 19) {
        icc_lut_args a{};
        float *samples[6] = {};
        for (int k = 0; k < 6; k++) {
            icc_lut_curve &c = k < 3 ? a.mc[k] : a.bc[k - 3];
            unsigned long long sample_offset, bits;
            if (fscanf(in, "%u %u %llu", &c.kind, &c.n, &sample_offset) != 3) return 66;
            for (int i = 0; i < 7; i++) {
                if (fscanf(in, "%llu", &bits) != 1) return 66;
                const uint64_t b64 = bits;
                memcpy(&c.q[i], &b64, 8);
            }
            if (c.kind == CE_ICC_LUT_CURVE_SAMPLED) {
                c.s = samples[k] = read_floats(tf, sample_offset, c.n);
                if (!c.s) return 69;
            }
            (k < 3 ? a.has_m : a.has_b) |= c.kind != CE_ICC_LUT_CURVE_IDENTITY;
        }
        const size_t bpp = ce_pixel_bytes_of(format), src_bytes = (size_t)n_px * bpp;
        const size_t slot_bytes = (size_t)n_px * 3 * (out_kind == 0 ? 4 : out_kind == 1 ? 1 : 2);
        if (bpp == 0 || out_kind < 0 || out_kind > 2) return 70;
        uint8_t *src = static_cast<uint8_t *>(malloc(src_bytes));
        if (!src || (reinterpret_cast<uintptr_t>(src) & 15) || fseek(sf, (long)src_offset, SEEK_SET) != 0 || fread(src, 1, src_bytes, sf) != src_bytes) return 67;
        float *table[3];
        for (int c = 0; c < 3; c++) {
            table[c] = read_floats(tf, table_offset + (unsigned long long)c * (maxv + 1ull), (size_t)maxv + 1);
            if (!table[c]) return 69;
        }
        float *clut = nullptr;
        if (g[0]) {
            clut = read_floats(tf, clut_offset, (size_t)g[0] * g[1] * g[2] * 4);
            if (!clut) return 69;
            a.clut = reinterpret_cast<const icc_lut_node *>(clut);
            a.s0 = g[1] * g[2], a.s1 = g[2];
            a.i0 = g[0] - 2, a.i1 = g[1] - 2, a.i2 = g[2] - 2;
            a.g0 = (float)(g[0] - 1), a.g1 = (float)(g[1] - 1), a.g2 = (float)(g[2] - 1);
        }
        float *mat = read_floats(tf, mat_offset, 12), *pcsm = read_floats(tf, pcsm_offset, 9);
        if (!mat || !pcsm) return 69;
        memcpy(a.mat, mat, 48);
        memcpy(a.c.m, pcsm, 36);
        a.has_matrix = (uint32_t)has_matrix, a.pcs = pcs;
        float *thr = nullptr;  // thr[k] = T[k] for k = 1 .. 2^depth_out - 1; entry 0 is the allocation's first float and is not read
        const size_t n_thr = ((size_t)1 << depth_out) - 1;
        if (out_kind != 0) {
            thr = static_cast<float *>(malloc((n_thr + 1) * 4));
            if (!thr || fseek(tf, (long)(thr_offset * 4), SEEK_SET) != 0 || fread(thr + 1, 4, n_thr, tf) != n_thr) return 69;
            thr[0] = 0.0f;
        }
        const size_t slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        void *dst = slab + off + (size_t)slot * slot_bytes;
        a.c.src = src, a.c.dst = out_kind == 0 ? static_cast<float *>(dst) : nullptr, a.c.n_pixels = (size_t)n_px, a.c.maxv = maxv;
        a.c.table = table[0], a.table_g = table[1], a.table_b = table[2];
        const uint32_t top = out_kind != 0 ? 1u << (depth_out - 1) : 0u;
        switch (format) {
            case CE_PIXEL_RGB8: run<CE_PIXEL_RGB8>(a, tetra != 0, out_kind, dst, thr, top); break;
            case CE_PIXEL_RGBA8: run<CE_PIXEL_RGBA8>(a, tetra != 0, out_kind, dst, thr, top); break;
            case CE_PIXEL_RGB16: run<CE_PIXEL_RGB16>(a, tetra != 0, out_kind, dst, thr, top); break;
            default: run<CE_PIXEL_RGBA16>(a, tetra != 0, out_kind, dst, thr, top); break;
        }
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        free(thr);
        free(mat);
        free(pcsm);
        free(clut);
        for (int c = 0; c < 3; c++) free(table[c]);
        for (int k = 0; k < 6; k++) free(samples[k]);
        free(src);
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(sf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
