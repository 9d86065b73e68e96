// The device code of the Delta E ITP maps (codec-eval_amd/csrc/hdr_fidelity_map_kernel.h, on top of hdr_fidelity_kernel.h)
// compiled for the host, as hdr_fidelity_kernel_host.cpp does for the scores: the HIP keywords are defined away, blockIdx /
// threadIdx / gridDim are plain variables that a loop sets, uint4 is a 16-byte aligned struct, atomicMax is a plain maximum -
// the threads run one after the other - and every thread of every block of the grid that hdrf_blocks, the launcher's own
// geometry, returns runs in turn: hdrf_stage for all 256 threads, then hdrf_map_lane for all 256.  The lanes' counts are added
// here; the block reduction of the kernel is shuffles, LDS and one atomic, which the GPU tests cover.  Built with
// -fsanitize=address,undefined and -ffp-contract=off by tests/test_delta_e_itp_map_kernel_host_cpu.py.  Everything is a heap
// block of exactly its size: the two slabs, the pair table, the thresholds, the coarse level, the LDS stand-in (refilled with a
// sentinel before every block), the map and the cell array.  An access outside any of them, or a misaligned 16-byte load or
// store, stops the run.
//
// usage: delta_e_itp_map_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth w h n_refs n_pairs  a[9] b[9] (float bits)  pair_ref[n_pairs]  thr[4]
// IN holds per case the 2^depth - 1 thresholds, the n_refs reference images and the n_pairs test images (floats).  Every case
// runs three times: the full map with counts, the cells of B = 8 with counts, counts alone.  OUT receives per case the map
// (u32 [n_pairs][h][w]), the cells (u32 [n_pairs][ceil(h / 8)][ceil(w / 8)]) and the three runs' counts (u64 [3][n_pairs][4]).
// stdout: one line "case N blocks wide|scalar" each, then "done N".
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

#include "hdr_fidelity_map_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

// one launch: counts[n_pairs][4] receives the sums of the lanes' counters
template <int DEPTH>
static void run(hdrf_args a, const hdrf_map_args &m, uint32_t n_pairs, uint32_t blocks, unsigned long long *counts)
{
    const size_t lds_floats = hdrf_coarse_len(DEPTH);
    float *lds = exact<float>(lds_floats);
    // two launches, as the launcher cuts a batch at a grid's y: pairs [0, half) and [half, n_pairs), the second with first = half
    const uint32_t half = n_pairs / 2;
    gridDim.x = blocks;
    for (uint32_t p = 0; p < n_pairs; p++) {
        unsigned long long t[kItpMaxThresholds] = {};
        for (uint32_t b = 0; b < blocks; b++) {
            a.first = p < half ? 0 : half, gridDim.y = p < half ? half : n_pairs - half;
            blockIdx.x = b, blockIdx.y = p - a.first;
            memset(lds, 0xff, lds_floats * sizeof(float));  // NaN: a threshold nothing is at or above
            for (unsigned th = 0; th < kHdrfThreads; th++) {
                threadIdx.x = th;
                hdrf_stage<DEPTH>(a, lds);
            }
            for (unsigned th = 0; th < kHdrfThreads; th++) {
                threadIdx.x = th;
                uint32_t cnt[kItpMaxThresholds];
                hdrf_map_lane<DEPTH>(a, m, lds, cnt);
                for (int j = 0; j < kItpMaxThresholds; j++) t[j] += cnt[j];
            }
        }
        for (int j = 4; j < kItpMaxThresholds; j++)
            if (t[j]) exit(71);  // the padding thresholds count nothing
        memcpy(counts + 4 * (size_t)p, t, 4 * sizeof(unsigned long long));
    }
    free(lds);
}

static void run_depth(unsigned depth, const hdrf_args &a, const hdrf_map_args &m, uint32_t n_pairs, uint32_t blocks, unsigned long long *counts)
{
    if (depth == 10) run<10>(a, m, n_pairs, blocks, counts);
    else if (depth == 12) run<12>(a, m, n_pairs, blocks, counts);
    else run<16>(a, m, n_pairs, blocks, counts);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned depth, w, h, n_refs, n_pairs;
    for (; fscanf(cfg, "%u %u %u %u %u", &depth, &w, &h, &n_refs, &n_pairs) == 5; cases++) {
        if ((depth != 10 && depth != 12 && depth != 16) || !w || !h || !n_refs || !n_pairs) return 66;
        hdrf_args a{};
        for (int i = 0; i < 18; i++) {
            uint32_t bits;
            if (fscanf(cfg, "%u", &bits) != 1) return 66;
            memcpy(i < 9 ? &a.a[i] : &a.b[i - 9], &bits, 4);
        }
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        hdrf_map_args m{};
        for (int j = 0; j < kItpMaxThresholds; j++) m.thr[j] = 0xffffffffu;
        for (int j = 0; j < 4; j++)
            if (fscanf(cfg, "%u", &m.thr[j]) != 1) return 66;
        const size_t n_pixels = (size_t)w * h, maxv = ((size_t)1 << depth) - 1, img = n_pixels * 3;
        float *table = exact<float>(maxv), *refs = exact<float>(n_refs * img), *tests = exact<float>(n_pairs * img);
        if (fread(table, 4, maxv, in) != maxv || fread(refs, 4, n_refs * img, in) != n_refs * img ||
            fread(tests, 4, n_pairs * img, in) != n_pairs * img)
            return 68;
        // the coarse level as the host runtime makes it: the table itself up to depth 12, every 16th threshold at 16
        const size_t n_coarse = hdrf_coarse_len((int)depth), stride = (size_t)1 << (depth - hdrf_coarse_bits((int)depth));
        float *coarse = exact<float>(n_coarse);
        for (size_t j = 0; j < n_coarse; j++) coarse[j] = table[(j + 1) * stride - 1];
        a.refs = refs, a.tests = tests, a.pair_ref = pair_ref, a.table = depth > 12 ? table : nullptr, a.coarse = coarse;
        a.n_pixels = n_pixels;
        a.denom = 4096.0 * (double)maxv;
        const uint32_t blocks = hdrf_blocks(n_pixels, n_pairs);
        unsigned long long *counts = exact<unsigned long long>(3 * 4 * (size_t)n_pairs);
        m.w = w;
        // the full map: every element is written, so it starts as a pattern no pixel of these cases has
        m.lb = 0, m.cw = w, m.pair_len = n_pixels;
        uint32_t *map = exact<uint32_t>(n_pairs * n_pixels);
        memset(map, 0xa5, n_pairs * n_pixels * sizeof(uint32_t));
        m.map = map;
        run_depth(depth, a, m, n_pairs, blocks, counts);
        // the cells of B = 8, zeroed as the launcher does
        m.lb = 3, m.cw = (w + 7) / 8, m.pair_len = (size_t)m.cw * ((h + 7) / 8);
        uint32_t *cells = exact<uint32_t>(n_pairs * m.pair_len);
        memset(cells, 0, n_pairs * m.pair_len * sizeof(uint32_t));
        m.map = cells;
        run_depth(depth, a, m, n_pairs, blocks, counts + 4 * (size_t)n_pairs);
        const size_t n_cells = n_pairs * m.pair_len;
        // counts alone
        m.map = nullptr;
        run_depth(depth, a, m, n_pairs, blocks, counts + 8 * (size_t)n_pairs);
        fwrite(map, sizeof(uint32_t), n_pairs * n_pixels, out);
        fwrite(cells, sizeof(uint32_t), n_cells, out);
        fwrite(counts, sizeof(unsigned long long), 3 * 4 * (size_t)n_pairs, out);
        printf("case %d %u %s\n", cases, blocks, (n_pixels & 3) ? "scalar" : "wide");
        free(cells), free(map), free(counts), free(coarse), free(tests), free(refs), free(table), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
