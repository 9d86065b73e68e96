// The device code of the fused Y'CbCr + CICP ingest (codec-eval_amd/csrc/yuv_cicp_kernel.h's k_yuv_tagged with cicp_pixel.h's
// cicp_px as its pixel, and the yuv_kernel.h it builds on) compiled for the host (hip_on_host.h): blockIdx / threadIdx are plain
// variables that a loop sets, and every thread of every block of a launch runs in turn.  Built with -ffp-contract=off
// -fsanitize=address,undefined by tests/test_yuv_cicp_kernel_host_cpu.py: each plane is allocated at exactly the bytes its
// rows need ((rows - 1) * pitch + row bytes), the table at maxv + 1 floats and the slab at exactly its size, `off` bytes after
// a 16-byte boundary with a guard in front, so a load outside a plane or the table or a store outside the slot stops the
// run, and so does a wide access to an address that is not a multiple of its width.
//
// usage: yuv_cicp_kernel_host CONFIGS TABLES OUT.  CONFIGS holds one case per line:
//   w h subsampling semiplanar triangle depth msb_aligned pad slot off seed KY KRV KGU KGV KBU y0 c0 maxv table_offset
//   has_matrix m[0] .. m[8]                                                  (the matrix as the bits of nine floats)
// TABLES is a file of floats; a case's table is maxv + 1 of them from table_offset on.  The slab holds slot + 1 slots and a
// trailing guard slot, filled with 0xEE bytes; the image goes to slot `slot`.  OUT receives, per case, the planes' rows
// without padding (Y, then CbCr or Cb and Cr) and then the slab.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "yuv_cicp_kernel.h"
#include "yuv_ladder.h"

// one launch: every thread of every block of ce_launch_yuv_tagged's grid
static void run(int bps, int sub, bool semi, const yuv_args &y, const cicp_args &c, bool matrix)
{
    const size_t groups = (size_t)((y.w + 7) / 8) * ((y.h + 1) / 2), blocks = (groups + 63) / 64;
    yuv_ladder(bps == 1, sub, semi, [&](auto b, auto s, auto sm) {
        constexpr int BPS = decltype(b)::value, SUB = decltype(s)::value;
        constexpr bool SEMI = decltype(sm)::value;
        for (size_t blk = 0; blk < blocks; blk++)
            for (unsigned t = 0; t < 64; t++) {
                blockIdx.x = (unsigned)blk, threadIdx.x = t;
                if (matrix) k_yuv_tagged<BPS, SUB, SEMI>(yuv_px_args<cicp_px<true>>{y, {c}});
                else k_yuv_tagged<BPS, SUB, SEMI>(yuv_px_args<cicp_px<false>>{y, {c}});
            }
    });
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *in = fopen(argv[1], "r"), *tf = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !tf || !out) return 65;
    int w, h, sub, semi, tri, d, msb, pad, off, has_matrix;
    unsigned long long slot, table_offset;
    unsigned seed, maxv;
    long long k[7];
    int cases = 0;
    while (fscanf(in, "%d %d %d %d %d %d %d %d %llu %d %u %lld %lld %lld %lld %lld %lld %lld %u %llu %d", &w, &h, &sub, &semi, &tri, &d, &msb,
                  &pad, &slot, &off, &seed, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5], &k[6], &maxv, &table_offset, &has_matrix) == 21) {
        cicp_args c{};
        for (int i = 0; i < 9; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&c.m[i], &bits, 4);
        }
        host_planes P;
        if (!make_planes(P, w, h, sub, semi, d, msb, pad, seed, out)) return 67;
        float *table = read_table(tf, table_offset, maxv);
        if (!table) return 69;
        const size_t slot_bytes = (size_t)w * h * 12, slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = make_slab(slab_bytes, off);
        if (!slab) return 68;
        yuv_args y{};
        fill_yuv_args(y, P, w, h, d, msb, tri, k, (int64_t)maxv);
        c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), c.table = table, c.maxv = maxv;
        run(d == 8 ? 1 : 2, sub, semi != 0, y, c, has_matrix != 0);
        if (!front_guard_intact(slab, off, cases)) return 2;
        fwrite(slab + off, 1, slab_bytes, out);
        free(slab);
        free(table);
        free_planes(P);
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
