// The device code of the fused Y'CbCr + ICC ingest (codec-eval_amd/csrc/yuv_icc_kernel.h's k_yuv_icc_encode and
// yuv_cicp_kernel.h's k_yuv_tagged, each with icc_pixel.h's icc_px or icc_lut_pixel.h's icc_lut_px as its pixel, and the
// yuv_kernel.h they build on) compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain variables that a loop sets,
// and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off -fsanitize=address,undefined by
// tests/test_yuv_icc_kernel_host_cpu.py: each plane is allocated at exactly the bytes its rows need ((rows - 1) * pitch + row
// bytes), each channel's table, the CLUT, each sampled curve, the thresholds and the slab at exactly their size, the slab `off`
// bytes after a 16-byte boundary with a guard in front, so a load outside a buffer or a store outside the slot stops the run,
// and so does a wide access to an address that is not a multiple of its width.  The thresholds' entry 0, which the search never
// reads, is poisoned: a read of it stops the run too.
//
// usage: yuv_icc_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line:
//   w h subsampling semiplanar triangle depth msb_aligned pad slot off seed KY KRV KGU KGV KBU y0 c0 maxv table_offset
//   out_kind depth_out thr_offset lut flag clut_offset g0 g1 g2 pcs lut_has_matrix mat_offset m_offset, then for each of the six
//   curves: kind n sample_offset q[0] .. q[6] (the bits of seven doubles)
// maxv = 2^rgb_depth - 1; out_kind: 0 packed f32, 1 packed u8, 2 packed u16; lut: 0 a matrix/TRC profile, whose flag says
// whether it has a matrix (m_offset: its nine floats) - the fields after it are then 0 - and 1 a LUT-based one, whose flag says
// tetrahedral (m_offset: f32(inv(A))); g0 = 0: no CLUT.  TABLES is a file of floats that the offsets count in.  The slab holds
// slot + 1 slots and a trailing guard slot, filled with 0xEE bytes; the image goes to slot `slot`.  OUT receives, per case, the
// planes' rows without padding (Y, then CbCr or Cb and Cr) and then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <sanitizer/asan_interface.h>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "yuv_icc_kernel.h"
#include "yuv_ladder.h"

// one launch: every thread of every block of ce_launch_yuv_icc's grid
template <class Pixel>
static void run(int bps, int sub, bool semi, const yuv_args &y, const Pixel &px, int out_kind, uint8_t *dst, const float *thr, uint32_t top)
{
    const size_t groups = (size_t)((y.w + 7) / 8) * ((y.h + 1) / 2), blocks = (groups + 63) / 64;
    yuv_ladder(bps == 1, sub, semi, [&](auto b, auto s, auto sm) {
        constexpr int BPS = decltype(b)::value, SUB = decltype(s)::value;
        constexpr bool SEMI = decltype(sm)::value;
        const yuv_icc_args<Pixel> k{y, px, dst, thr, top};
        for (size_t blk = 0; blk < blocks; blk++)
            for (unsigned t = 0; t < 64; t++) {
                blockIdx.x = (unsigned)blk, threadIdx.x = t;
                if (out_kind == 0) k_yuv_tagged<BPS, SUB, SEMI>(yuv_px_args<Pixel>{y, px});
                else if (out_kind == 1) k_yuv_icc_encode<BPS, false, SUB, SEMI>(k);
                else k_yuv_icc_encode<BPS, true, SUB, SEMI>(k);
            }
    });
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
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    int w, h, sub, semi, tri, d, msb, pad, off, out_kind, lut, flag, lut_has_matrix;
    unsigned long long slot, table_offset, thr_offset, clut_offset, mat_offset, m_offset;
    unsigned seed, maxv, depth_out, g[3], pcs;
    long long k[7];
    int cases = 0;
    while (fscanf(in, "%d %d %d %d %d %d %d %d %llu %d %u %lld %lld %lld %lld %lld %lld %lld %u %llu %d %u %llu %d %d %llu %u %u %u %u %d %llu %llu", &w, &h, &sub,
                  &semi, &tri, &d, &msb, &pad, &slot, &off, &seed, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5], &k[6], &maxv, &table_offset, &out_kind, &depth_out,
                  &thr_offset, &lut, &flag, &clut_offset, &g[0], &g[1], &g[2], &pcs, &lut_has_matrix, &mat_offset, &m_offset) == 33) {
        icc_lut_args a{};  // its c, table_g and table_b are all the matrix/TRC pixel takes
        float *samples[6] = {};
        for (int i = 0; i < 6; i++) {
            icc_lut_curve &c = i < 3 ? a.mc[i] : a.bc[i - 3];
            unsigned long long sample_offset, bits;
            if (fscanf(in, "%u %u %llu", &c.kind, &c.n, &sample_offset) != 3) return 66;
            for (int q = 0; q < 7; q++) {
                if (fscanf(in, "%llu", &bits) != 1) return 66;
                const uint64_t b64 = bits;
                memcpy(&c.q[q], &b64, 8);
            }
            if (c.kind == CE_ICC_LUT_CURVE_SAMPLED) {
                c.s = samples[i] = read_floats(tf, sample_offset, c.n);
                if (!c.s) return 69;
            }
            (i < 3 ? a.has_m : a.has_b) |= c.kind != CE_ICC_LUT_CURVE_IDENTITY;
        }
        if (out_kind < 0 || out_kind > 2) return 70;
        host_planes P;
        if (!make_planes(P, w, h, sub, semi, d, msb, pad, seed, out)) return 67;
        float *table[3];
        for (int c = 0; c < 3; c++) {
            table[c] = read_floats(tf, table_offset + (unsigned long long)c * (maxv + 1ull), (size_t)maxv + 1);
            if (!table[c]) return 69;
        }
        float *clut = nullptr, *mat = nullptr;
        if (lut && g[0]) {
            clut = read_floats(tf, clut_offset, (size_t)g[0] * g[1] * g[2] * 4);
            if (!clut) return 69;
            a.clut = reinterpret_cast<const icc_lut_node *>(clut);
            a.s0 = g[1] * g[2], a.s1 = g[2];
            a.i0 = g[0] - 2, a.i1 = g[1] - 2, a.i2 = g[2] - 2;
            a.g0 = (float)(g[0] - 1), a.g1 = (float)(g[1] - 1), a.g2 = (float)(g[2] - 1);
        }
        if (lut) {
            mat = read_floats(tf, mat_offset, 12);
            if (!mat) return 69;
            memcpy(a.mat, mat, 48);
            a.has_matrix = (uint32_t)lut_has_matrix, a.pcs = pcs;
        }
        float *m = read_floats(tf, m_offset, 9);
        if (!m) return 69;
        memcpy(a.c.m, m, 36);
        // thr[k] = T[k] for k = 1 .. 2^depth_out - 1.  Entry 0 is never read: it is the second half of an 8-byte granule of
        // its own, poisoned, and T[1] starts the next granule
        float *thr_raw = nullptr, *thr = nullptr;
        const size_t n_thr = ((size_t)1 << depth_out) - 1;
        if (out_kind != 0) {
            thr_raw = static_cast<float *>(malloc((n_thr + 2) * 4));
            if (!thr_raw || (reinterpret_cast<uintptr_t>(thr_raw) & 7) || fseek(tf, (long)(thr_offset * 4), SEEK_SET) != 0 || fread(thr_raw + 2, 4, n_thr, tf) != n_thr)
                return 69;
            thr = thr_raw + 1;
            ASAN_POISON_MEMORY_REGION(thr_raw, 8);
        }
        const size_t slot_bytes = (size_t)w * h * 3 * (out_kind == 0 ? 4 : out_kind == 1 ? 1 : 2), slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        uint8_t *dst = slab + off + (size_t)slot * slot_bytes;
        yuv_args y{};
        fill_yuv_args(y, P, w, h, d, msb, tri, k, (int64_t)maxv);
        a.c.dst = out_kind == 0 ? reinterpret_cast<float *>(dst) : nullptr, a.c.maxv = maxv;
        a.c.table = table[0], a.table_g = table[1], a.table_b = table[2];
        const uint32_t top = out_kind != 0 ? 1u << (depth_out - 1) : 0u;
        const int bps = d == 8 ? 1 : 2;
        if (lut) {
            if (flag) run(bps, sub, semi != 0, y, icc_lut_px<true>{a}, out_kind, dst, thr, top);
            else run(bps, sub, semi != 0, y, icc_lut_px<false>{a}, out_kind, dst, thr, top);
        } else {
            const icc_args ia{a.c, a.table_g, a.table_b};
            if (flag) run(bps, sub, semi != 0, y, icc_px<true>{ia}, out_kind, dst, thr, top);
            else run(bps, sub, semi != 0, y, icc_px<false>{ia}, out_kind, dst, thr, top);
        }
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        if (thr_raw) ASAN_UNPOISON_MEMORY_REGION(thr_raw, 8);
        free(thr_raw);
        free(m);
        free(mat);
        free(clut);
        for (int c = 0; c < 3; c++) free(table[c]);
        for (int i = 0; i < 6; i++) free(samples[i]);
        free_planes(P);
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
