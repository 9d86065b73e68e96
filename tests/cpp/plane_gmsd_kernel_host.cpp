// The device code of GMSD (codec-eval_amd/csrc/plane_gmsd_kernel.h, with plane_fidelity_kernel.h's planes, sample rule and wide
// loads) compiled for the host, as plane_hvs_kernel_host.cpp does for PSNR-HVS: the HIP keywords are defined away, blockIdx /
// threadIdx are plain variables that a loop sets, and every thread of every block of the launcher's own grid runs in turn,
// phase by phase as the barrier orders a block on the device - gmsd_stage for all 256 threads, then gmsd_score for all 256.  A
// thread block's five integers are combined here as the kernel combines them - four sums and a maximum - and the host's
// finishing (gmsd_finish) is the header's own.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_plane_gmsd_kernel_host_cpu.py.  Everything is a heap block of exactly its size: every plane (pitch padding between
// its rows only, none after the last row) at a 16-byte aligned address plus the offset its image asks for, the tables, and the
// LDS stand-in, which is refilled with 0xff bytes before every block so that a value the stage did not write shows.
//
// usage: plane_gmsd_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth w h subsampling n_refs n_pairs pair_ref[n_pairs] then per image (references, then tests): layout msb_aligned offset
//   pitch[stored planes]
// IN holds per case and image the stored planes, each (rows - 1) * pitch + row bytes long; OUT receives per case and pair, per
// plane, 5 u64 (sum_q, sum_q2 low, sum_q2 high, n_pos, max_dis) and 2 f64 (gmsd, gmsm).  stdout: one line "case N thread_blocks
// dead_blocks wide_rows" each, then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "plane_gmsd_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

template <class SAMPLE>
static void run(gmsd_args a, uint32_t n_pairs, unsigned long long *out, unsigned long *thread_blocks, unsigned long *dead)
{
    gmsd_lds *lds = exact<gmsd_lds>(1);
    const uint64_t w2 = ((uint64_t)a.w[0] + 1) / 2, h2 = ((uint64_t)a.h[0] + 1) / 2;
    gridDim.x = (unsigned)(((w2 + kGmsdTileW - 1) / kGmsdTileW) * ((h2 + kGmsdTileH - 1) / kGmsdTileH));  // plane_gmsd.hip: ce_yuv_plane_gmsd
    gridDim.y = n_pairs * a.n_planes;
    a.first = 0;
    for (uint32_t by = 0; by < gridDim.y; by++)
        for (uint32_t bx = 0; bx < gridDim.x; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(lds, 0xff, sizeof(gmsd_lds));
            for (unsigned th = 0; th < kGmsdThreads; th++) threadIdx.x = th, gmsd_stage<SAMPLE>(a, *lds);
            gmsd_part t{};
            for (unsigned th = 0; th < kGmsdThreads; th++) {
                threadIdx.x = th;
                const gmsd_part q = gmsd_score(a, *lds);
                t.q += q.q, t.hh += q.hh, t.hl += q.hl, t.ll += q.ll;
                t.max_dis = q.max_dis > t.max_dis ? q.max_dis : t.max_dis;
            }
            threadIdx.x = 0;
            const gmsd_where o = gmsd_tile(a);
            ++*thread_blocks;
            if (!o.live) {
                ++*dead;
                if (t.q || t.hh || t.hl || t.ll || t.max_dis) exit(71);  // a dead block adds nothing
                continue;
            }
            unsigned long long *acc = out + (size_t)o.pair * kGmsdOut + (size_t)o.plane * kGmsdTerms;
            acc[0] += t.q, acc[1] += t.hh, acc[2] += t.hl, acc[3] += t.ll;
            acc[4] = t.max_dis > acc[4] ? t.max_dis : acc[4];
        }
    free(lds);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned depth, w, h, sub, n_refs, n_pairs;
    for (; fscanf(cfg, "%u %u %u %u %u %u", &depth, &w, &h, &sub, &n_refs, &n_pairs) == 6; cases++) {
        if ((depth != 8 && depth != 10 && depth != 12) || !w || !h || sub > 3 || !n_refs || !n_pairs) return 66;
        const uint32_t n_planes = sub == 3 ? 1 : 3, bps = depth == 8 ? 1 : 2;
        const uint32_t cw = sub == 0 ? w : (w + 1) / 2, ch = sub == 2 ? (h + 1) / 2 : h;
        uint32_t *pair_ref = exact<uint32_t>(n_pairs);
        for (unsigned i = 0; i < n_pairs; i++)
            if (fscanf(cfg, "%u", &pair_ref[i]) != 1 || pair_ref[i] >= n_refs) return 66;
        const size_t n_img = (size_t)n_refs + n_pairs;
        pf_plane *tab = exact<pf_plane>(n_img * 3);
        std::vector<void *> blocks;
        unsigned long wide_rows = 0;
        for (size_t i = 0; i < n_img; i++) {
            unsigned layout, msb, offset;
            if (fscanf(cfg, "%u %u %u", &layout, &msb, &offset) != 3 || layout > 1 || (msb && depth == 8) || offset >= 16 || offset % bps) return 66;
            const unsigned n_stored = sub == 3 ? 1 : layout ? 2 : 3;
            uint8_t *base[3] = {};
            size_t pitch[3] = {};
            for (unsigned s = 0; s < n_stored; s++) {
                const size_t rows = s ? ch : h, row = (size_t)(s == 0 ? w : layout ? 2 * cw : cw) * bps;
                unsigned long long pt;
                if (fscanf(cfg, "%llu", &pt) != 1 || pt < row) return 66;
                const size_t len = (rows - 1) * pt + row;
                // the plane starts `offset` bytes into a 16-byte aligned block and ends it
                void *block = nullptr;
                if (posix_memalign(&block, 16, offset + len)) return 70;
                blocks.push_back(block);
                base[s] = static_cast<uint8_t *>(block) + offset, pitch[s] = pt;
                if (fread(base[s], 1, len, in) != len) return 68;
                for (size_t r = 0; r < rows; r++) wide_rows += reinterpret_cast<uintptr_t>(base[s] + r * pt) % 16 == 0;
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
        unsigned long long *res = exact<unsigned long long>((size_t)n_pairs * kGmsdOut);
        memset(res, 0, sizeof(unsigned long long) * n_pairs * kGmsdOut);
        gmsd_args a{};
        a.tab = tab, a.pair_ref = pair_ref, a.out = nullptr;
        a.n_refs = n_refs, a.n_planes = n_planes, a.maxv = (1u << depth) - 1u;
        a.k = 24480ull << (2 * (depth - 8));
        for (uint32_t p = 0; p < n_planes; p++) a.w[p] = p ? cw : w, a.h[p] = p ? ch : h;
        unsigned long thread_blocks = 0, dead = 0;
        if (bps == 1) run<uint8_t>(a, n_pairs, res, &thread_blocks, &dead);
        else run<uint16_t>(a, n_pairs, res, &thread_blocks, &dead);
        for (unsigned i = 0; i < n_pairs; i++)
            for (uint32_t p = 0; p < n_planes; p++) {
                const gmsd_plane_result f = gmsd_finish(res + (size_t)i * kGmsdOut + (size_t)p * kGmsdTerms, a.w[p], a.h[p]);
                const uint64_t ints[5] = {f.sum_q, f.sum_q2[0], f.sum_q2[1], f.n_pos, f.max_dis};
                const double dbl[2] = {f.gmsd, f.gmsm};
                fwrite(ints, sizeof(uint64_t), 5, out), fwrite(dbl, sizeof(double), 2, out);
            }
        printf("case %d %lu %lu %lu\n", cases, thread_blocks, dead, wide_rows);
        for (void *b : blocks) free(b);
        free(res), free(tab), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
