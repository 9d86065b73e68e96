// The device code of the alpha compositor (codec-eval_amd/csrc/alpha_kernel.h) compiled for the host: the HIP keywords are
// defined away, blockIdx / threadIdx are plain variables that a loop sets, and every thread of every block of a launch runs
// in turn.  Built with -fsanitize=address,undefined by tests/test_alpha_kernel_host_cpu.py: the source is allocated at
// exactly its size and the K slots at exactly theirs, `off` bytes after a 16-byte boundary with a guard in front, so a load
// outside the source or a store outside the slots stops the run, and so does a wide store to an address that is not a
// multiple of its width.
//
// usage: alpha_kernel_host CONFIGS OUT.  CONFIGS holds one case per line:
//   form depth n_pixels K off seed bg[0][0] bg[0][1] bg[0][2] ... bg[K-1][2]
// form 0: RGBA8 -> u8 slots, 1: RGBA8 -> u16 slots, 2: RGBA16 -> u16 slots.  OUT receives, per case, the source and then
// the K slots.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

#include "alpha_kernel.h"

template <bool SRC16, bool DST16, int DEPTH>
static void run(const alpha_args &a)
{
    const size_t groups = a.n_pixels / (DST16 ? 8 : 16), blocks = std::max<size_t>((groups + kAlphaBlock - 1) / kAlphaBlock, 1);  // ce_launch_alpha's grid
    for (size_t b = 0; b < blocks; b++)
        for (unsigned t = 0; t < (unsigned)kAlphaBlock; t++) {
            blockIdx.x = (unsigned)b, threadIdx.x = t;
            k_alpha<SRC16, DST16, DEPTH>(a);
        }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 64;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 65;
    int form, depth, K, off;
    unsigned long long n_px;
    unsigned seed;
    int cases = 0;
    while (fscanf(in, "%d %d %llu %d %d %u", &form, &depth, &n_px, &K, &off, &seed) == 6) {
        alpha_args a{};
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 3; c++)
                if (fscanf(in, "%u", &a.bg[k][c]) != 1) return 66;
        const bool src16 = form == 2, dst16 = form != 0;
        const size_t src_bytes = (size_t)n_px * 4 * (src16 ? 2 : 1), slot_bytes = (size_t)n_px * 3 * (dst16 ? 2 : 1);
        auto next = [&seed] { return seed = seed * 1664525u + 1013904223u; };
        uint8_t *src = static_cast<uint8_t *>(malloc(src_bytes));
        if (!src || (reinterpret_cast<uintptr_t>(src) & 15)) return 67;  // malloc: 16-byte aligned, as the staging buffer is
        for (size_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)(next() >> 24);
        const uint32_t m = (1u << depth) - 1u;
        for (size_t p = 0; p < n_px; p++) {  // alpha 0 and m well represented; u16: in range but one sample in 16 above it
            const unsigned sel = next() >> 30;
            if (src16) {
                uint16_t v[4];
                memcpy(v, src + 8 * p, 8);
                for (int c = 0; c < 4; c++)
                    if ((next() >> 28) != 0) v[c] &= (uint16_t)m;
                if (sel == 0) v[3] = 0;
                if (sel == 1) v[3] = (uint16_t)m;
                memcpy(src + 8 * p, v, 8);
            } else {
                if (sel == 0) src[4 * p + 3] = 0;
                if (sel == 1) src[4 * p + 3] = 255;
            }
        }
        fwrite(src, 1, src_bytes, out);
        uint8_t *slab = static_cast<uint8_t *>(malloc(K * slot_bytes + (size_t)off));  // malloc: 16-byte aligned
        if (!slab || (reinterpret_cast<uintptr_t>(slab) & 15)) return 68;
        memset(slab, 0xEE, K * slot_bytes + (size_t)off);
        a.src = src, a.dst = slab + off, a.slot_bytes = slot_bytes, a.n_pixels = (size_t)n_px, a.n_bg = (uint32_t)K;
        if (form == 0) run<false, false, 8>(a);
        else if (form == 1) run<false, true, 8>(a);
        else if (depth == 8) run<true, true, 8>(a);
        else if (depth == 10) run<true, true, 10>(a);
        else if (depth == 12) run<true, true, 12>(a);
        else run<true, true, 16>(a);
        for (int i = 0; i < off; i++)
            if (slab[i] != 0xEE) {
                fprintf(stderr, "case %d wrote in front of its slots\n", cases);
                return 2;
            }
        fwrite(slab + off, 1, K * slot_bytes, out);
        free(slab);
        free(src);
        cases++;
    }
    fclose(in);
    fclose(out);
    printf("%d\n", cases);
    return 0;
}
