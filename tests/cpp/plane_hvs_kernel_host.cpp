// The device code of PSNR-HVS / PSNR-HVS-M (codec-eval_amd/csrc/plane_hvs_kernel.h, with plane_fidelity_kernel.h's planes and
// sample rule) compiled for the host, as plane_fidelity_kernel_host.cpp does for the plane-domain scores: the HIP keywords are
// defined away, blockIdx / threadIdx are plain variables that a loop sets, and every thread of every block of the launcher's
// own grid runs in turn, phase by phase as the two barriers order a block on the device - hvs_rows for all 256 threads, then
// hvs_columns for all 256, then hvs_score for all 256, each thread's column held between the last two as its registers hold
// it.  A thread block's two integers are added here and handed over as the kernel hands them over: low and high 32 bits into
// two accumulators each.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_plane_hvs_kernel_host_cpu.py.  Everything is a heap block of exactly its size: every plane (pitch padding between
// its rows only, none after the last row), the tables, and the LDS stand-in, which is refilled with NaN before every block.
//
// usage: plane_hvs_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth w h subsampling n_refs n_pairs step pair_ref[n_pairs] then per image (references, then tests): layout msb_aligned
//   pitch[stored planes]
// IN holds per case and image the stored planes, each (rows - 1) * pitch + row bytes long; OUT receives per case n_pairs x 12
// u64: [plane][hvs, hvsm][low, high].  stdout: one line "case N thread_blocks dead_threads" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "plane_hvs_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

// JPEG Annex K, table K.1
static const int kAnnexK[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};

template <class SAMPLE>
static void run(hvs_args a, uint32_t n_pairs, unsigned long long *out, unsigned long *thread_blocks, unsigned long *dead)
{
    hvs_lds *lds = exact<hvs_lds>(1);
    hvs_cols *cols = exact<hvs_cols>(kHvsThreads);
    const uint64_t n0 = (uint64_t)((a.w[0] - 8) / a.step + 1) * ((a.h[0] - 8) / a.step + 1);
    gridDim.x = (unsigned)((n0 + kHvsBlocks - 1) / kHvsBlocks), gridDim.y = n_pairs * a.n_planes;  // plane_hvs.hip: ce_yuv_plane_hvs
    a.first = 0;
    for (uint32_t by = 0; by < gridDim.y; by++)
        for (uint32_t bx = 0; bx < gridDim.x; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(lds, 0xff, sizeof(hvs_lds));
            memset(cols, 0xff, sizeof(hvs_cols) * kHvsThreads);
            for (unsigned th = 0; th < kHvsThreads; th++) threadIdx.x = th, hvs_rows<SAMPLE>(a, *lds);
            for (unsigned th = 0; th < kHvsThreads; th++) threadIdx.x = th, hvs_columns(a, *lds, cols[th]);
            unsigned long long t[2] = {0, 0};
            for (unsigned th = 0; th < kHvsThreads; th++) {
                threadIdx.x = th;
                unsigned long long q[2];
                hvs_score(a, *lds, cols[th], q);
                t[0] += q[0], t[1] += q[1];
                if (!hvs_block(a).live) ++*dead;
            }
            threadIdx.x = 0;
            const hvs_where o = hvs_block(a);
            for (int m = 0; m < 2; m++) {
                unsigned long long *acc = out + (size_t)o.pair * kHvsOut + ((size_t)o.plane * 2 + m) * 2;
                acc[0] += t[m] & 0xffffffffull, acc[1] += t[m] >> 32;
            }
            ++*thread_blocks;
        }
    free(lds), free(cols);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    double *tables = exact<double>(128);
    for (int i = 0; i < 64; i++) tables[i] = 25.73509 / (double)kAnnexK[i], tables[64 + i] = 100.0 / (double)(kAnnexK[i] * kAnnexK[i]);
    int cases = 0;
    unsigned depth, w, h, sub, n_refs, n_pairs, step;
    for (; fscanf(cfg, "%u %u %u %u %u %u %u", &depth, &w, &h, &sub, &n_refs, &n_pairs, &step) == 7; cases++) {
        if ((depth != 8 && depth != 10 && depth != 12) || w < 8 || h < 8 || sub > 3 || !n_refs || !n_pairs || step < 1 || step > 8) return 66;
        const uint32_t n_planes = sub == 3 ? 1 : 3, bps = depth == 8 ? 1 : 2;
        const uint32_t cw = sub == 0 ? w : (w + 1) / 2, ch = sub == 2 ? (h + 1) / 2 : h;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t n_img = (size_t)n_refs + n_pairs;
        pf_plane *tab = exact<pf_plane>(n_img * 3);
        std::vector<uint8_t *> blocks;
        for (size_t i = 0; i < n_img; i++) {
            unsigned layout, msb;
            if (fscanf(cfg, "%u %u", &layout, &msb) != 2 || layout > 1 || (msb && depth == 8)) return 66;
            const unsigned n_stored = sub == 3 ? 1 : layout ? 2 : 3;
            uint8_t *base[3] = {};
            size_t pitch[3] = {};
            for (unsigned s = 0; s < n_stored; s++) {
                const size_t rows = s ? ch : h, row = (size_t)(s == 0 ? w : layout ? 2 * cw : cw) * bps;
                unsigned long long pt;
                if (fscanf(cfg, "%llu", &pt) != 1 || pt < row) return 66;
                const size_t len = (rows - 1) * pt + row;
                base[s] = exact<uint8_t>(len), pitch[s] = pt;
                if (fread(base[s], 1, len, in) != len) return 68;
                blocks.push_back(base[s]);
            }
            for (uint32_t p = 0; p < 3; p++) {
                pf_plane e{};
                if (p < n_planes) {
                    const unsigned s = layout && p == 2 ? 1 : p;
                    e.base = base[s] + (layout && p == 2 ? bps : 0), e.pitch = pitch[s], e.step = layout && p ? 2 : 1, e.shift = msb ? 16 - depth : 0;
                }
                tab[i * 3 + p] = e;
            }
        }
        unsigned long long *res = exact<unsigned long long>((size_t)n_pairs * kHvsOut);
        memset(res, 0, sizeof(unsigned long long) * n_pairs * kHvsOut);
        hvs_args a{};
        a.tab = tab, a.pair_ref = pair_ref, a.csf = tables, a.mc = tables + 64, a.out = nullptr;
        a.n_refs = n_refs, a.n_planes = n_planes, a.maxv = (1u << depth) - 1u, a.step = step;
        a.unit = (double)(1ull << (36 - 2 * depth));
        for (uint32_t p = 0; p < n_planes; p++) a.w[p] = p ? cw : w, a.h[p] = p ? ch : h;
        unsigned long thread_blocks = 0, dead = 0;
        if (bps == 1) run<uint8_t>(a, n_pairs, res, &thread_blocks, &dead);
        else run<uint16_t>(a, n_pairs, res, &thread_blocks, &dead);
        fwrite(res, sizeof(unsigned long long), (size_t)n_pairs * kHvsOut, out);
        printf("case %d %lu %lu\n", cases, thread_blocks, dead);
        for (uint8_t *b : blocks) free(b);
        free(res), free(tab), free(pair_ref);
    }
    free(tables);
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
