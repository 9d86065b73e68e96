// The device code of the Y'CbCr ingest (codec-eval_amd/csrc/yuv_kernel.h) compiled for the host: the HIP keywords are
// defined away, blockIdx / threadIdx are plain variables that a loop sets, and every thread of every block of a launch runs
// in turn.  Built with -fsanitize=address,undefined by tests/test_yuv_kernel_host_cpu.py: each plane is allocated at exactly
// the bytes its rows need ((rows - 1) * pitch + row bytes) and the slot at exactly its size plus a guard in front, so a load
// outside a plane or a store outside the slot stops the run.
//
// usage: yuv_kernel_host CONFIGS OUT.  CONFIGS holds one case per line:
//   w h subsampling semiplanar triangle depth msb_aligned depth_out out16 pad slot_offset seed KY KRV KGU KGV KBU y0 c0
// OUT receives, per case, the planes' rows without padding (Y, then CbCr or Cb and Cr) and then the converted image.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"
#include "ingest_host.h"

#include "yuv_kernel.h"
#include "yuv_ladder.h"

// one launch: every thread of every block of ce_launch_yuv's grid
static void run(int bps, bool out16, int sub, bool semi, const yuv_args &a, uint8_t *dst)
{
    const size_t groups = (size_t)((a.w + 7) / 8) * ((a.h + 1) / 2), blocks = (groups + 63) / 64;
    yuv_ladder(bps == 1, sub, semi, [&](auto b, auto s, auto sm) {
        constexpr int BPS = decltype(b)::value, SUB = decltype(s)::value;
        constexpr bool SEMI = decltype(sm)::value;
        for (size_t blk = 0; blk < blocks; blk++)
            for (unsigned t = 0; t < 64; t++) {
                blockIdx.x = (unsigned)blk, threadIdx.x = t;
                if (out16) k_yuv<BPS, true, SUB, SEMI>(a, dst);
                else k_yuv<BPS, false, SUB, SEMI>(a, dst);
            }
    });
}

int main(int argc, char **argv)
{
    if (argc != 3) return 64;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 65;
    int w, h, sub, semi, tri, d, msb, D, out16, pad, off;
    unsigned seed;
    long long k[7];
    int cases = 0;
    while (fscanf(in, "%d %d %d %d %d %d %d %d %d %d %d %u %lld %lld %lld %lld %lld %lld %lld", &w, &h, &sub, &semi, &tri, &d, &msb, &D,
                  &out16, &pad, &off, &seed, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5], &k[6]) == 19) {
        host_planes P;
        if (!make_planes(P, w, h, sub, semi, d, msb, pad, seed, out)) return 67;
        const size_t out_bytes = (size_t)w * h * 3 * (out16 ? 2 : 1);
        uint8_t *slab = static_cast<uint8_t *>(malloc(out_bytes + (size_t)off));
        memset(slab, 0xEE, out_bytes + (size_t)off);
        yuv_args a{};
        fill_yuv_args(a, P, w, h, d, msb, tri, k, ((int64_t)1 << D) - 1);
        run(d == 8 ? 1 : 2, out16 != 0, sub, semi != 0, a, slab + off);
        for (int i = 0; i < off; i++)
            if (slab[i] != 0xEE) {
                fprintf(stderr, "case %d wrote in front of its slot\n", cases);
                return 2;
            }
        fwrite(slab + off, 1, out_bytes, out);
        free(slab);
        free_planes(P);
        cases++;
    }
    fclose(in);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
