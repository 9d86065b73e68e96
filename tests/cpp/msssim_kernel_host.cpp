// The device code of SSIM / MS-SSIM (codec-eval_amd/csrc/msssim_kernel.h) compiled for the host, as hdr_fidelity_kernel_host.cpp
// does for the HDR fidelity scores: the HIP keywords are defined away, blockIdx / threadIdx / gridDim are plain variables that
// a loop sets, and every thread of every block of the launcher's own grids runs in turn - per level mss_stage for all 256
// threads, then mss_columns for all 256, then mss_lane for all 256, as the two barriers order a block on the device; between
// levels mss_pool_sample for every sample of the next level of every slot.  The lanes' integers are added here in the order the
// loop meets them; they are integers, so the order does not matter.  Built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_msssim_kernel_host_cpu.py.  Everything is a heap block of exactly its size: the two slabs, the
// pair table, every level of the pyramid, and the two LDS stand-ins, which are refilled with NaN before every block so that
// what a previous block staged cannot stand in for what this block did not.  A load outside any of them, or a misaligned
// 16-byte load, stops the run.
//
// usage: msssim_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   bytes_per_sample depth w h n_refs n_pairs levels pair_ref[n_pairs]
// IN holds per case the n_refs reference images and the n_pairs test images (packed RGB, u8 or u16); OUT receives per case
// n_pairs x [5][3][2] i64: ssim_q, cs_q.  stdout: one line "case N tiles_of_level_0" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

#include "msssim_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

template <class SAMPLE>
static void run_level(const mss_args &a, uint32_t tiles, uint32_t n_pairs, long long *out)
{
    float *s_in = static_cast<float *>(aligned_alloc(16, 2 * kMssInLen * sizeof(float)));
    double *s_col = static_cast<double *>(aligned_alloc(16, kMssStreams * kMssColLen * sizeof(double)));
    if (!s_in || !s_col) exit(70);
    gridDim.x = tiles, gridDim.y = 3 * n_pairs;
    for (uint32_t by = 0; by < 3 * n_pairs; by++)
        for (uint32_t bx = 0; bx < tiles; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(s_in, 0xff, 2 * kMssInLen * sizeof(float));
            memset(s_col, 0xff, kMssStreams * kMssColLen * sizeof(double));
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_stage<SAMPLE>(a, s_in);
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_columns(s_in, s_col);
            for (unsigned th = 0; th < kMssThreads; th++) {
                threadIdx.x = th;
                long long acc[2];
                mss_lane(a, s_col, acc);
                long long *o = out + (((size_t)(by / 3) * 5 + a.level) * 3 + by % 3) * 2;
                o[0] += acc[0], o[1] += acc[1];
            }
        }
    free(s_in), free(s_col);
}

template <class SAMPLE>
static void run_pool(mss_pool_args a, uint32_t n_slots)
{
    a.first = 0;
    for (uint32_t s = 0; s < n_slots; s++) {
        blockIdx.y = s;
        for (size_t i = 0; i < (size_t)3 * a.ow * a.oh; i++) mss_pool_sample<SAMPLE>(a, i);
    }
}

template <class SAMPLE>
static uint32_t run_case(const SAMPLE *refs, const SAMPLE *tests, const uint32_t *pair_ref, uint32_t depth, uint32_t w, uint32_t h,
                         uint32_t n_refs, uint32_t n_pairs, uint32_t levels, long long *out)
{
    const double maxv = (double)((1u << depth) - 1u);
    const void *cur[2] = {refs, tests};
    float *owned[2] = {nullptr, nullptr};
    uint32_t tiles0 = 0;
    for (uint32_t l = 0; l < levels; l++) {
        const size_t plane = (size_t)w * h;
        mss_args g{};
        g.refs = cur[0], g.tests = cur[1], g.ref_slot = g.test_slot = 3 * plane, g.chan = l ? plane : 1, g.px = l ? 1 : 3;
        g.pair_ref = pair_ref, g.w = w, g.h = h, g.level = l, g.first = 0;
        g.tiles_x = (w - kMssHalo + kMssTileW - 1) / kMssTileW;
        const uint32_t tiles = g.tiles_x * ((h - kMssHalo + kMssTileH - 1) / kMssTileH);
        g.c1 = (0.01 * maxv) * (0.01 * maxv), g.c2 = (0.03 * maxv) * (0.03 * maxv);
        if (l) run_level<float>(g, tiles, n_pairs, out);
        else run_level<SAMPLE>(g, tiles, n_pairs, out), tiles0 = tiles;
        if (l + 1 == levels) break;
        const uint32_t ow = (w + (w & 1u)) / 2, oh = (h + (h & 1u)) / 2;
        float *next[2];
        for (int side = 0; side < 2; side++) {
            const uint32_t n_slots = side ? n_pairs : n_refs;
            next[side] = exact<float>((size_t)n_slots * 3 * ow * oh);
            mss_pool_args p{};
            p.src = cur[side], p.dst = next[side], p.src_slot = 3 * plane, p.dst_slot = (size_t)3 * ow * oh;
            p.chan = g.chan, p.px = g.px, p.w = w, p.h = h, p.ow = ow, p.oh = oh;
            if (l) run_pool<float>(p, n_slots);
            else run_pool<SAMPLE>(p, n_slots);
        }
        for (int side = 0; side < 2; side++) free(owned[side]), owned[side] = next[side], cur[side] = next[side];
        w = ow, h = oh;
    }
    free(owned[0]), free(owned[1]);
    return tiles0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned bps, depth, w, h, n_refs, n_pairs, levels;
    for (; fscanf(cfg, "%u %u %u %u %u %u %u", &bps, &depth, &w, &h, &n_refs, &n_pairs, &levels) == 7; cases++) {
        if ((bps != 1 && bps != 2) || depth > 8 * bps || depth < 8 || w < 11 || h < 11 || !n_refs || !n_pairs || (levels != 1 && levels != 5)) return 66;
        if (levels == 5 && (w <= 160 || h <= 160)) return 66;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t img = (size_t)w * h * 3;
        uint8_t *refs = exact<uint8_t>(n_refs * img * bps), *tests = exact<uint8_t>(n_pairs * img * bps);
        if (fread(refs, bps, n_refs * img, in) != n_refs * img || fread(tests, bps, n_pairs * img, in) != n_pairs * img) return 68;
        long long *res = exact<long long>((size_t)n_pairs * 30);
        memset(res, 0, sizeof(long long) * n_pairs * 30);
        const uint32_t tiles = bps == 1 ? run_case<uint8_t>(refs, tests, pair_ref, depth, w, h, n_refs, n_pairs, levels, res)
                                        : run_case<uint16_t>(reinterpret_cast<uint16_t *>(refs), reinterpret_cast<uint16_t *>(tests), pair_ref,
                                                             depth, w, h, n_refs, n_pairs, levels, res);
        fwrite(res, sizeof(long long), (size_t)n_pairs * 30, out);
        printf("case %d %u\n", cases, tiles);
        free(res), free(tests), free(refs), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
