// The device code of the SSIM / MS-SSIM maps (codec-eval_amd/csrc/msssim_map_kernel.h, on top of msssim_kernel.h) compiled for the
// host, as msssim_kernel_host.cpp does for the scores: the HIP keywords are defined away, blockIdx / threadIdx / gridDim are plain
// variables that a loop sets, atomicMax is a plain maximum - the threads run one after the other - and every thread of every
// block of the launcher's own grids runs in turn, phase by phase as the barriers order a block on the device: mss_stage for all
// 256 threads, then mss_columns, then mss_map_lane, and for cells mss_map_rows and mss_map_cells; before that mss_pool_sample
// for every sample of every level up to the one asked for.  The lanes' counts are added here; the block reduction of the kernel
// is shuffles, LDS and one atomic, which the GPU tests cover.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_msssim_map_kernel_host_cpu.py.  Everything is a heap block of exactly its size: the two slabs, the pair table,
// every level of the pyramid, the LDS stand-ins (refilled with 0xff before every block), the map and the cell arrays.  The map
// and the cells that are written whole start as a pattern no position of the cases has, the cells that take atomics as zeros,
// as the launcher leaves them.  An access outside any of them, or a misaligned 8- or 16-byte access, stops the run.
//
// usage: msssim_map_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   bytes_per_sample depth w h n_refs n_pairs levels level what thr[8] pair_ref[n_pairs]
// IN holds per case the n_refs reference images and the n_pairs test images (packed RGB, u8 or u16).  Every case runs eight
// times: the full map with counts, the cells of B = 2 .. 64 without, counts alone.  OUT receives per case the map (u32 [n_pairs]
// [3][vh][vw]), the six cell arrays (u32 [n_pairs][3][ceil(vh / B)][ceil(vw / B)]) and the two runs' counts (u64 [2][n_pairs][3]
// [8]).  stdout: one line "case N tiles aligned_rows|odd_rows" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

static inline uint32_t atomicMax(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    if (v > old) *p = v;
    return old;
}

#include "msssim_map_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

// one launch: counts[n_pairs][3][8] receives the sums of the lanes' counters; nullptr: the launch has no thresholds but the
// padding, and the counters must stay zero
template <class SAMPLE>
static void run_map(const mss_args &a, const mss_map_args &m, uint32_t tiles, uint32_t n_pairs, unsigned long long *counts)
{
    float *s_in = static_cast<float *>(aligned_alloc(16, 2 * kMssInLen * sizeof(float)));
    double *s_col = static_cast<double *>(aligned_alloc(16, kMssStreams * kMssColLen * sizeof(double)));
    uint32_t *s_park = exact<uint32_t>(kMssParkLen), *s_rows = exact<uint32_t>(kMssParkLen);
    if (!s_in || !s_col) exit(70);
    gridDim.x = tiles, gridDim.y = 3 * n_pairs;
    for (uint32_t by = 0; by < 3 * n_pairs; by++) {
        unsigned long long t[kMssMapMaxThresholds] = {};
        for (uint32_t bx = 0; bx < tiles; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(s_in, 0xff, 2 * kMssInLen * sizeof(float));
            memset(s_col, 0xff, kMssStreams * kMssColLen * sizeof(double));
            memset(s_park, 0xff, kMssParkLen * sizeof(uint32_t));
            memset(s_rows, 0xff, kMssParkLen * sizeof(uint32_t));
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_stage<SAMPLE>(a, s_in);
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_columns(s_in, s_col);
            for (unsigned th = 0; th < kMssThreads; th++) {
                threadIdx.x = th;
                uint32_t cnt[kMssMapMaxThresholds];
                mss_map_lane(a, m, s_col, s_park, cnt);
                for (int j = 0; j < kMssMapMaxThresholds; j++) t[j] += cnt[j];
            }
            if (m.map && m.lb) {
                for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_map_rows(m, s_park, s_rows);
                for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_map_cells(a, m, s_rows);
            }
        }
        if (counts) memcpy(counts + (size_t)by * kMssMapMaxThresholds, t, sizeof(t));
        for (int j = 0; !counts && j < kMssMapMaxThresholds; j++)
            if (t[j]) exit(71);  // thresholds of 2^32 - 1 count nothing
    }
    free(s_rows), free(s_park), free(s_col), free(s_in);
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
                         uint32_t n_refs, uint32_t n_pairs, uint32_t level, uint32_t what, const uint32_t *thr, FILE *out, bool *odd_rows)
{
    const double maxv = (double)((1u << depth) - 1u);
    const void *cur[2] = {refs, tests};
    float *owned[2] = {nullptr, nullptr};
    for (uint32_t l = 0; l < level; l++) {
        const size_t plane = (size_t)w * h;
        const uint32_t ow = (w + (w & 1u)) / 2, oh = (h + (h & 1u)) / 2;
        float *next[2];
        for (int side = 0; side < 2; side++) {
            const uint32_t n_slots = side ? n_pairs : n_refs;
            next[side] = exact<float>((size_t)n_slots * 3 * ow * oh);
            mss_pool_args p{};
            p.src = cur[side], p.dst = next[side], p.src_slot = 3 * plane, p.dst_slot = (size_t)3 * ow * oh;
            p.chan = l ? plane : 1, p.px = l ? 1 : 3, p.w = w, p.h = h, p.ow = ow, p.oh = oh;
            if (l) run_pool<float>(p, n_slots);
            else run_pool<SAMPLE>(p, n_slots);
        }
        for (int side = 0; side < 2; side++) free(owned[side]), owned[side] = next[side], cur[side] = next[side];
        w = ow, h = oh;
    }
    const size_t plane = (size_t)w * h;
    mss_args g{};
    g.refs = cur[0], g.tests = cur[1], g.ref_slot = g.test_slot = 3 * plane, g.chan = level ? plane : 1, g.px = level ? 1 : 3;
    g.pair_ref = pair_ref, g.w = w, g.h = h, g.level = level, g.first = 0;
    const uint32_t vw = w - kMssHalo, vh = h - kMssHalo;
    g.tiles_x = (vw + kMssTileW - 1) / kMssTileW;
    const uint32_t tiles = g.tiles_x * ((vh + kMssTileH - 1) / kMssTileH);
    g.c1 = (0.01 * maxv) * (0.01 * maxv), g.c2 = (0.03 * maxv) * (0.03 * maxv);
    *odd_rows = (vw & 1u) != 0;
    const size_t n_counts = (size_t)n_pairs * 3 * kMssMapMaxThresholds;
    unsigned long long *counts = exact<unsigned long long>(2 * n_counts);
    for (uint32_t lb = 0; lb <= 7; lb++) {  // 7: counts alone
        mss_map_args m{};
        m.what = what, m.lb = lb < 7 ? lb : 0;
        m.cw = (vw + (1u << m.lb) - 1) >> m.lb, m.ch = (vh + (1u << m.lb) - 1) >> m.lb;
        for (int j = 0; j < kMssMapMaxThresholds; j++) m.thr[j] = lb == 0 || lb == 7 ? thr[j] : 0xffffffffu;
        const size_t len = lb < 7 ? (size_t)n_pairs * 3 * m.cw * m.ch : 0;
        uint32_t *map = lb < 7 ? exact<uint32_t>(len) : nullptr;
        if (map) memset(map, lb >= 5 ? 0 : 0xa5, len * sizeof(uint32_t));
        m.map = map;
        unsigned long long *c = lb == 0 ? counts : lb == 7 ? counts + n_counts : nullptr;
        if (level) run_map<float>(g, m, tiles, n_pairs, c);
        else run_map<SAMPLE>(g, m, tiles, n_pairs, c);
        if (map) fwrite(map, sizeof(uint32_t), len, out);
        free(map);
    }
    fwrite(counts, sizeof(unsigned long long), 2 * n_counts, out);
    free(counts), free(owned[0]), free(owned[1]);
    return tiles;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned bps, depth, w, h, n_refs, n_pairs, levels, level, what;
    for (; fscanf(cfg, "%u %u %u %u %u %u %u %u %u", &bps, &depth, &w, &h, &n_refs, &n_pairs, &levels, &level, &what) == 9; cases++) {
        if ((bps != 1 && bps != 2) || depth > 8 * bps || depth < 8 || w < 11 || h < 11 || !n_refs || !n_pairs || (levels != 1 && levels != 5)) return 66;
        if ((levels == 5 && (w <= 160 || h <= 160)) || level >= levels || what > 1) return 66;
        uint32_t thr[kMssMapMaxThresholds];
        for (int j = 0; j < kMssMapMaxThresholds; j++)
            if (fscanf(cfg, "%u", &thr[j]) != 1) return 66;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t img = (size_t)w * h * 3;
        uint8_t *refs = exact<uint8_t>(n_refs * img * bps), *tests = exact<uint8_t>(n_pairs * img * bps);
        if (fread(refs, bps, n_refs * img, in) != n_refs * img || fread(tests, bps, n_pairs * img, in) != n_pairs * img) return 68;
        bool odd_rows = false;
        const uint32_t tiles = bps == 1 ? run_case<uint8_t>(refs, tests, pair_ref, depth, w, h, n_refs, n_pairs, level, what, thr, out, &odd_rows)
                                        : run_case<uint16_t>(reinterpret_cast<uint16_t *>(refs), reinterpret_cast<uint16_t *>(tests), pair_ref,
                                                             depth, w, h, n_refs, n_pairs, level, what, thr, out, &odd_rows);
        printf("case %d %u %s\n", cases, tiles, odd_rows ? "odd_rows" : "aligned_rows");
        free(tests), free(refs), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
