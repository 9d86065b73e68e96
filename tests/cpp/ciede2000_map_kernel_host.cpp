// The device code of the CIEDE2000 maps (codec-eval_amd/csrc/ciede2000_map_kernel.h, on top of ciede2000_kernel.h and the
// ciede2000_pixel.h they run) compiled for the host, as ciede2000_kernel_host.cpp does for the scores: the HIP keywords are
// defined away, blockIdx / threadIdx / gridDim are plain variables that a loop sets, uint4 is a 16-byte aligned struct,
// atomicMax is a plain maximum - the threads run one after the other - and every thread of every block of the grid that
// cie_blocks, the launcher's own geometry, returns runs in turn: cie_stage for all 256 threads, then cie_map_lane for all 256.
// The lanes' counts are added here; the block reduction of the kernel is shuffles, LDS and one atomic, which the GPU tests
// cover.  Built with -fsanitize=address,undefined and -ffp-contract=off by tests/test_ciede2000_map_kernel_host_cpu.py.
// Everything is a heap block of exactly its size: the two slabs, the pair table, the two sRGB tables, the LDS stand-in (as long
// as the launcher's dynamic LDS and refilled with NaN before every block), the map and the cell arrays.  An access outside any
// of them, or a misaligned 16-byte load or store, stops the run.
//
// usage: ciede2000_map_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   deep depth_ref depth_test w h n_refs n_pairs what  thr[8]  pair_ref[n_pairs]  n_blocks block[n_blocks]
// IN holds per case the two tables (2^depth floats each), the n_refs reference images and the n_pairs test images (u8 samples
// with deep = 0, else u16).  Every case runs 2 + n_blocks times: the full map with counts, the cells of every block with counts,
// counts alone.  OUT receives per case the map (u32 [n_pairs][h][w]), per block the cells (u32 [n_pairs][ceil(h / B)][ceil(w /
// B)]) and the runs' counts (u64 [2 + n_blocks][n_pairs][8]: full, the blocks in turn, alone).  stdout: one line
// "case N blocks wide|scalar lds_floats" each, then "done N".
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

#include "ciede2000_map_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

// one launch: counts[n_pairs][8] receives the sums of the lanes' counters
template <bool DEEP>
static void run(cie_args a, const cie_map_args &m, uint32_t n_pairs, uint32_t blocks, unsigned long long *counts)
{
    const size_t lds_floats = cie_lds_floats(a.depth[0], a.depth[1]);
    float *lds = exact<float>(lds_floats);
    // two launches, as the launcher cuts a batch at a grid's y: pairs [0, half) and [half, n_pairs), the second with first = half
    const uint32_t half = n_pairs / 2;
    gridDim.x = blocks;
    for (uint32_t p = 0; p < n_pairs; p++) {
        unsigned long long t[kCieMaxThresholds] = {};
        for (uint32_t b = 0; b < blocks; b++) {
            a.first = p < half ? 0 : half, gridDim.y = p < half ? half : n_pairs - half;
            blockIdx.x = b, blockIdx.y = p - a.first;
            memset(lds, 0xff, lds_floats * sizeof(float));  // NaN
            for (unsigned th = 0; th < kCieThreads; th++) {
                threadIdx.x = th;
                cie_stage(a, lds);
            }
            for (unsigned th = 0; th < kCieThreads; th++) {
                threadIdx.x = th;
                uint32_t cnt[kCieMaxThresholds];
                cie_map_lane<DEEP>(a, m, lds, cnt);
                for (int j = 0; j < kCieMaxThresholds; j++) t[j] += cnt[j];
            }
        }
        memcpy(counts + (size_t)kCieMaxThresholds * p, t, sizeof(t));
    }
    free(lds);
}

static void run_kind(bool deep, const cie_args &a, const cie_map_args &m, uint32_t n_pairs, uint32_t blocks, unsigned long long *counts)
{
    if (deep) run<true>(a, m, n_pairs, blocks, counts);
    else run<false>(a, m, n_pairs, blocks, counts);
}

static bool depth_ok(unsigned d) { return d == 8 || d == 10 || d == 12 || d == 16; }

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned deep, depth[2], w, h, n_refs, n_pairs, what;
    for (; fscanf(cfg, "%u %u %u %u %u %u %u %u", &deep, &depth[0], &depth[1], &w, &h, &n_refs, &n_pairs, &what) == 8; cases++) {
        if (deep > 1 || !depth_ok(depth[0]) || !depth_ok(depth[1]) || (!deep && (depth[0] != 8 || depth[1] != 8)) || !w || !h || !n_refs || !n_pairs ||
            what > kCieMapDh)
            return 66;
        cie_args a{};
        for (int j = 0; j < kCieMaxThresholds; j++)
            if (fscanf(cfg, "%u", &a.thr[j]) != 1) return 66;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        unsigned n_blocks, block[8];
        if (fscanf(cfg, "%u", &n_blocks) != 1 || n_blocks > 8) return 66;
        for (unsigned i = 0; i < n_blocks; i++)
            if (fscanf(cfg, "%u", &block[i]) != 1 || block[i] < 2 || block[i] > 64 || (block[i] & (block[i] - 1))) return 66;
        const size_t n_pixels = (size_t)w * h;
        const size_t len[2] = {(size_t)1 << depth[0], (size_t)1 << depth[1]}, img = n_pixels * 3 * (deep ? 2 : 1);
        float *table[2] = {exact<float>(len[0]), exact<float>(len[1])};
        uint8_t *refs = exact<uint8_t>(n_refs * img), *tests = exact<uint8_t>(n_pairs * img);
        if (fread(table[0], 4, len[0], in) != len[0] || fread(table[1], 4, len[1], in) != len[1] || fread(refs, 1, n_refs * img, in) != n_refs * img ||
            fread(tests, 1, n_pairs * img, in) != n_pairs * img)
            return 68;
        a.refs = refs, a.tests = tests, a.pair_ref = pair_ref, a.table[0] = table[0], a.table[1] = table[1];
        a.depth[0] = depth[0], a.depth[1] = depth[1], a.n_pixels = n_pixels;
        const uint32_t blocks = cie_blocks(n_pixels, n_pairs, deep != 0);
        const size_t per_run = (size_t)kCieMaxThresholds * n_pairs;
        unsigned long long *counts = exact<unsigned long long>((2 + n_blocks) * per_run);
        cie_map_args m{};
        m.what = what, m.w = w;
        // the full map: every element is written, so it starts as a pattern no pixel of these cases has
        m.lb = 0, m.cw = w, m.pair_len = n_pixels;
        uint32_t *map = exact<uint32_t>(n_pairs * n_pixels);
        memset(map, 0xa5, n_pairs * n_pixels * sizeof(uint32_t));
        m.map = map;
        run_kind(deep != 0, a, m, n_pairs, blocks, counts);
        fwrite(map, sizeof(uint32_t), n_pairs * n_pixels, out);
        free(map);
        // the cells of every block, zeroed as the launcher does
        for (unsigned i = 0; i < n_blocks; i++) {
            m.lb = 0;
            while ((1u << m.lb) < block[i]) m.lb++;
            m.cw = (w + block[i] - 1) >> m.lb, m.pair_len = (size_t)m.cw * ((h + block[i] - 1) >> m.lb);
            uint32_t *cells = exact<uint32_t>(n_pairs * m.pair_len);
            memset(cells, 0, n_pairs * m.pair_len * sizeof(uint32_t));
            m.map = cells;
            run_kind(deep != 0, a, m, n_pairs, blocks, counts + (1 + i) * per_run);
            fwrite(cells, sizeof(uint32_t), n_pairs * m.pair_len, out);
            free(cells);
        }
        // counts alone
        m.map = nullptr, m.lb = 0, m.cw = w, m.pair_len = n_pixels;
        run_kind(deep != 0, a, m, n_pairs, blocks, counts + (1 + n_blocks) * per_run);
        fwrite(counts, sizeof(unsigned long long), (2 + n_blocks) * per_run, out);
        printf("case %d %u %s %u\n", cases, blocks, cie_wide(n_pixels, deep != 0) ? "wide" : "scalar", cie_lds_floats(depth[0], depth[1]));
        free(counts), free(tests), free(refs), free(table[1]), free(table[0]), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
