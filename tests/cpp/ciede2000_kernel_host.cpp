// The device code of the CIEDE2000 scores (codec-eval_amd/csrc/ciede2000_kernel.h with the ciede2000_pixel.h it runs) compiled
// for the host, as hdr_fidelity_kernel_host.cpp does for the HDR fidelity scores: the HIP keywords are defined away, blockIdx /
// threadIdx / gridDim are plain variables that a loop sets, and every thread of every block of the grid that cie_blocks - the
// launcher's own geometry - returns runs in turn: cie_stage for all 256 threads, then cie_lane for all 256, as the barrier
// between them orders a block on the device.  The lanes' integers are added (and, the second, maximised) here, in the order
// the loop meets them; they are integers, so the order does not matter.  Built with -fsanitize=address,undefined and
// -ffp-contract=off by tests/test_ciede2000_kernel_host_cpu.py.  Everything is a heap block of exactly its size: the two slabs,
// the pair table, the two sRGB tables and the LDS stand-in, which is as long as the launcher's dynamic LDS and is refilled with
// NaN before every block so that a table a previous block staged cannot stand in for one this block did not.  A load outside
// any of them, or a misaligned 16-byte load, stops the run.
//
// usage: ciede2000_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   deep depth_ref depth_test n_pixels n_refs n_pairs  thr[8]  pair_ref[n_pairs]
// IN holds per case the two tables (2^depth floats each), the n_refs reference images and the n_pairs test images (u8 samples
// with deep = 0, else u16); OUT receives per case n_pairs x 10 u64: sum_q20, max_q20, n_above[8].  stdout: one line
// "case N blocks wide|scalar lds_floats" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

#include "ciede2000_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

template <bool DEEP>
static void run(cie_args a, uint32_t n_pairs, uint32_t blocks, unsigned long long *out)
{
    const size_t lds_floats = cie_lds_floats(a.depth[0], a.depth[1]);
    float *lds = exact<float>(lds_floats);
    // two launches, as the launcher cuts a batch at a grid's y: pairs [0, half) and [half, n_pairs), the second with first = half
    const uint32_t half = n_pairs / 2;
    gridDim.x = blocks;
    for (uint32_t p = 0; p < n_pairs; p++) {
        unsigned long long t[kCieOut] = {};
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
                cie_acc acc;
                cie_lane<DEEP>(a, lds, acc);
                t[0] += acc.sum;
                t[1] = acc.max > t[1] ? acc.max : t[1];
                for (int j = 0; j < kCieMaxThresholds; j++) t[2 + j] += acc.cnt[j];
            }
        }
        memcpy(out + (size_t)kCieOut * p, t, sizeof(t));
    }
    free(lds);
}

static bool depth_ok(unsigned d) { return d == 8 || d == 10 || d == 12 || d == 16; }

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned deep, depth[2], n_refs, n_pairs;
    unsigned long long n_pixels;
    for (; fscanf(cfg, "%u %u %u %llu %u %u", &deep, &depth[0], &depth[1], &n_pixels, &n_refs, &n_pairs) == 6; cases++) {
        if (deep > 1 || !depth_ok(depth[0]) || !depth_ok(depth[1]) || (!deep && (depth[0] != 8 || depth[1] != 8)) || !n_pixels || !n_refs || !n_pairs)
            return 66;
        cie_args a{};
        for (int j = 0; j < kCieMaxThresholds; j++)
            if (fscanf(cfg, "%u", &a.thr[j]) != 1) return 66;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t len[2] = {(size_t)1 << depth[0], (size_t)1 << depth[1]}, img = (size_t)n_pixels * 3 * (deep ? 2 : 1);
        float *table[2] = {exact<float>(len[0]), exact<float>(len[1])};
        uint8_t *refs = exact<uint8_t>(n_refs * img), *tests = exact<uint8_t>(n_pairs * img);
        if (fread(table[0], 4, len[0], in) != len[0] || fread(table[1], 4, len[1], in) != len[1] || fread(refs, 1, n_refs * img, in) != n_refs * img ||
            fread(tests, 1, n_pairs * img, in) != n_pairs * img)
            return 68;
        a.refs = refs, a.tests = tests, a.pair_ref = pair_ref, a.table[0] = table[0], a.table[1] = table[1];
        a.depth[0] = depth[0], a.depth[1] = depth[1], a.n_pixels = n_pixels;
        const uint32_t blocks = cie_blocks(n_pixels, n_pairs, deep != 0);
        unsigned long long *res = exact<unsigned long long>((size_t)kCieOut * n_pairs);
        if (deep) run<true>(a, n_pairs, blocks, res);
        else run<false>(a, n_pairs, blocks, res);
        fwrite(res, sizeof(unsigned long long), (size_t)kCieOut * n_pairs, out);
        printf("case %d %u %s %u\n", cases, blocks, cie_wide(n_pixels, deep != 0) ? "wide" : "scalar", cie_lds_floats(depth[0], depth[1]));
        free(res), free(tests), free(refs), free(table[1]), free(table[0]), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
