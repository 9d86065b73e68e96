// The device code of the HDR fidelity scores (codec-eval_amd/csrc/hdr_fidelity_kernel.h) compiled for the host, as
// resample_f32_kernel_host.cpp does for the float resampler: the HIP keywords are defined away, blockIdx / threadIdx / gridDim
// are plain variables that a loop sets, and every thread of every block of the grid that hdrf_blocks - the launcher's own
// geometry - returns runs in turn: hdrf_stage for all 256 threads, then hdrf_lane for all 256, as the barrier between them
// orders a block on the device.  The lanes' integers are added (and, the third, maximised) here, in the order the loop meets
// them; they are integers, so the order does not matter.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_hdr_fidelity_kernel_host_cpu.py.  Everything is a heap block of exactly its size: the two slabs, the pair table,
// the thresholds, the coarse level made from them and the LDS stand-in, which is refilled with a sentinel before every block
// so that thresholds a previous block staged cannot stand in for ones this block did not.  A load outside any of them, or a
// misaligned 16-byte load, stops the run.
//
// usage: hdr_fidelity_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth n_pixels n_refs n_pairs  a[9] b[9] (float bits)  pair_ref[n_pairs]
// IN holds per case the 2^depth - 1 thresholds, the n_refs reference images and the n_pairs test images (floats); OUT receives
// per case n_pairs x 3 u64: pq_sse, itp_sum_q20, itp_max_q20.  stdout: one line "case N blocks wide|scalar" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hip_on_host.h"

#include "hdr_fidelity_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

template <int DEPTH>
static void run(hdrf_args a, uint32_t n_pairs, uint32_t blocks, unsigned long long *out)
{
    const size_t lds_floats = hdrf_coarse_len(DEPTH);
    float *lds = exact<float>(lds_floats);
    // two launches, as the launcher cuts a batch at a grid's y: pairs [0, half) and [half, n_pairs), the second with first = half
    const uint32_t half = n_pairs / 2;
    gridDim.x = blocks;
    for (uint32_t p = 0; p < n_pairs; p++) {
        unsigned long long t[3] = {0, 0, 0};
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
                unsigned long long acc[3];
                hdrf_lane<DEPTH>(a, lds, acc);
                t[0] += acc[0], t[1] += acc[1];
                t[2] = acc[2] > t[2] ? acc[2] : t[2];
            }
        }
        memcpy(out + 3 * (size_t)p, t, sizeof(t));
    }
    free(lds);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned depth, n_refs, n_pairs;
    unsigned long long n_pixels;
    for (; fscanf(cfg, "%u %llu %u %u", &depth, &n_pixels, &n_refs, &n_pairs) == 4; cases++) {
        if ((depth != 10 && depth != 12 && depth != 16) || !n_pixels || !n_refs || !n_pairs) return 66;
        hdrf_args a{};
        for (int i = 0; i < 18; i++) {
            uint32_t bits;
            if (fscanf(cfg, "%u", &bits) != 1) return 66;
            memcpy(i < 9 ? &a.a[i] : &a.b[i - 9], &bits, 4);
        }
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t maxv = ((size_t)1 << depth) - 1, img = (size_t)n_pixels * 3;
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
        unsigned long long *res = exact<unsigned long long>(3 * (size_t)n_pairs);
        if (depth == 10) run<10>(a, n_pairs, blocks, res);
        else if (depth == 12) run<12>(a, n_pairs, blocks, res);
        else run<16>(a, n_pairs, blocks, res);
        fwrite(res, sizeof(unsigned long long), 3 * (size_t)n_pairs, out);
        printf("case %d %u %s\n", cases, blocks, (n_pixels & 3) ? "scalar" : "wide");
        free(res), free(coarse), free(tests), free(refs), free(table), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
