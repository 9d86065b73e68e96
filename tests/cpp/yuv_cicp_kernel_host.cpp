// The device code of the fused Y'CbCr + CICP ingest (codec-eval_amd/csrc/yuv_cicp_kernel.h, with the yuv_kernel.h and
// cicp_kernel.h it builds on) compiled for the host: the HIP keywords are defined away, blockIdx / threadIdx are plain
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

#include "yuv_cicp_kernel.h"

template <int BPS, int SUB, bool SEMI>
static void run(const yuv_cicp_args &a, bool matrix)
{
    const size_t groups = (size_t)((a.y.w + 7) / 8) * ((a.y.h + 1) / 2), blocks = (groups + 63) / 64;  // ce_launch_yuv_cicp's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < 64; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            if (matrix) k_yuv_cicp<BPS, SUB, SEMI, true>(a); else k_yuv_cicp<BPS, SUB, SEMI, false>(a);
        }
}
template <int BPS, int SUB>
static void run_layout(bool semi, const yuv_cicp_args &a, bool matrix)
{
    if (semi && SUB != CE_YUV_400) run<BPS, SUB, true>(a, matrix);
    else run<BPS, SUB, false>(a, matrix);
}
template <int BPS>
static void run_sub(int sub, bool semi, const yuv_cicp_args &a, bool matrix)
{
    switch (sub) {
        case CE_YUV_444: run_layout<BPS, CE_YUV_444>(semi, a, matrix); break;
        case CE_YUV_422: run_layout<BPS, CE_YUV_422>(semi, a, matrix); break;
        case CE_YUV_420: run_layout<BPS, CE_YUV_420>(semi, a, matrix); break;
        default: run_layout<BPS, CE_YUV_400>(semi, a, matrix); break;
    }
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
        yuv_cicp_args a{};
        for (int i = 0; i < 9; i++) {
            uint32_t bits;
            if (fscanf(in, "%u", &bits) != 1) return 66;
            memcpy(&a.c.m[i], &bits, 4);
        }
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
        float *table = static_cast<float *>(malloc(((size_t)maxv + 1) * 4));
        if (!table || fseek(tf, (long)(table_offset * 4), SEEK_SET) != 0 || fread(table, 4, (size_t)maxv + 1, tf) != (size_t)maxv + 1) return 69;
        const size_t slot_bytes = (size_t)w * h * 12, slab_bytes = (size_t)(slot + 2) * slot_bytes;
        uint8_t *slab = static_cast<uint8_t *>(malloc(slab_bytes + (size_t)off));  // malloc: 16-byte aligned
        if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15)) return 68;
        memset(slab, 0xEE, slab_bytes + (size_t)off);
        yuv_args &y = a.y;
        y.p0 = plane[0], y.p1 = plane[1], y.p2 = plane[2];
        y.pitch0 = pitch[0], y.pitch1 = pitch[1], y.pitch2 = pitch[2];
        y.w = (uint32_t)w, y.h = (uint32_t)h, y.cw = (uint32_t)cw, y.ch = (uint32_t)ch;
        y.shift = msb ? 16u - (uint32_t)d : 0u, y.maxv = (1u << d) - 1u, y.triangle = tri;
        y.ky = k[0], y.krv = k[1], y.kgu = k[2], y.kgv = k[3], y.kbu = k[4], y.y0 = k[5], y.c0 = k[6];
        y.m = (int64_t)maxv;
        a.c.dst = reinterpret_cast<float *>(slab + off + (size_t)slot * slot_bytes), a.c.table = table, a.c.maxv = maxv;
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
        cases++;
    }
    fclose(in);
    fclose(tf);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
