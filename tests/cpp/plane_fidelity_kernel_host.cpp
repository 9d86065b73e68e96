// The device code of the plane-domain scores (codec-eval_amd/csrc/plane_fidelity_kernel.h, with the parts of msssim_kernel.h it
// reuses) compiled for the host, as msssim_kernel_host.cpp does for SSIM / MS-SSIM: the HIP keywords are defined away,
// blockIdx / threadIdx / gridDim are plain variables that a loop sets, and every thread of every block of the launcher's own
// grids runs in turn - pf_sse_thread for all 256 threads of a block of k_plane_sse; per level pf_stage for all 256 threads, then
// mss_columns for all 256, then mss_lane for all 256, as the two barriers order a block on the device; between levels
// pf_pool_sample for every sample of the next level of every image.  The integers are added here in the order the loop meets
// them; they are integers, so the order does not matter.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_plane_fidelity_kernel_host_cpu.py.  Everything is a heap block of exactly its size: every plane (pitch padding
// between its rows only, none after the last row), the tables, every level of the pyramid, and the two LDS stand-ins, which are
// refilled with NaN before every block.  A load outside any of them, or a misaligned 16-byte load, stops the run.
//
// usage: plane_fidelity_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth w h subsampling n_refs n_pairs levels pair_ref[n_pairs] then per image (references, then tests): layout msb_aligned
//   pitch[stored planes]
// IN holds per case and image the stored planes, each (rows - 1) * pitch + row bytes long; OUT receives per case n_pairs x 33
// i64: sse[3], then [plane][level][2] = ssim_q, cs_q.  stdout: one line "case N wide_rows scalar_rows level0_tiles" each, then
// "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "plane_fidelity_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

struct geometry {
    uint32_t n_refs, n_pairs, n_planes, bps, maxv;
    uint32_t lw[3][5], lh[3][5], n_levels[3];
};

template <int BPS>
static void run_sse(const geometry &g, const pf_plane *tab, const uint32_t *pair_ref, long long *out)
{
    pf_sse_args a{};
    a.tab = tab, a.pair_ref = pair_ref, a.out = nullptr, a.n_refs = g.n_refs, a.n_planes = g.n_planes, a.maxv = g.maxv, a.first = 0;
    for (uint32_t p = 0; p < g.n_planes; p++) a.w[p] = g.lw[p][0], a.h[p] = g.lh[p][0];
    const uint32_t blocks = std::min((a.h[0] + kPfWaves - 1) / kPfWaves, std::max(64u, 4096u / g.n_pairs));  // plane_fidelity.hip: launch
    gridDim.x = blocks, gridDim.y = g.n_pairs * g.n_planes;
    for (uint32_t by = 0; by < gridDim.y; by++)
        for (uint32_t bx = 0; bx < blocks; bx++)
            for (unsigned th = 0; th < kPfThreads; th++) {
                blockIdx.x = bx, blockIdx.y = by, threadIdx.x = th;
                const pf_where o = pf_sse_block(a);
                out[(size_t)o.pair * kPfOut + o.plane] += (long long)pf_sse_thread<BPS>(a);
            }
}

template <class SAMPLE>
static uint32_t run_level(pf_level_args a, uint32_t n_pairs, long long *out)
{
    float *s_in = static_cast<float *>(aligned_alloc(16, 2 * kMssInLen * sizeof(float)));
    double *s_col = static_cast<double *>(aligned_alloc(16, kMssStreams * kMssColLen * sizeof(double)));
    if (!s_in || !s_col) exit(70);
    a.m.tiles_x = (a.m.w - kMssHalo + kMssTileW - 1) / kMssTileW;
    const uint32_t tiles = a.m.tiles_x * ((a.m.h - kMssHalo + kMssTileH - 1) / kMssTileH);
    gridDim.x = tiles, gridDim.y = n_pairs;
    for (uint32_t by = 0; by < n_pairs; by++)
        for (uint32_t bx = 0; bx < tiles; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(s_in, 0xff, 2 * kMssInLen * sizeof(float));
            memset(s_col, 0xff, kMssStreams * kMssColLen * sizeof(double));
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, pf_stage<SAMPLE>(a, s_in);
            for (unsigned th = 0; th < kMssThreads; th++) threadIdx.x = th, mss_columns(s_in, s_col);
            for (unsigned th = 0; th < kMssThreads; th++) {
                threadIdx.x = th;
                long long acc[2];
                mss_lane(a.m, s_col, acc);
                long long *o = out + (size_t)by * kPfOut + 3 + ((size_t)a.plane * 5 + a.m.level) * 2;
                o[0] += acc[0], o[1] += acc[1];
            }
        }
    free(s_in), free(s_col);
    return tiles;
}

template <class SAMPLE>
static void run_pool(pf_pool_args a, uint32_t n_img)
{
    a.first = 0;
    for (uint32_t s = 0; s < n_img; s++) {
        blockIdx.y = s;
        for (size_t i = 0; i < (size_t)a.ow * a.oh; i++) pf_pool_sample<SAMPLE>(a, i);
    }
}

template <class SAMPLE>
static uint32_t run_levels(const geometry &g, const pf_plane *tab, const uint32_t *pair_ref, long long *out)
{
    const double maxv = (double)g.maxv;
    const uint32_t n_img = g.n_refs + g.n_pairs;
    uint32_t tiles0 = 0;
    for (uint32_t p = 0; p < g.n_planes; p++) {
        float *cur = nullptr;
        for (uint32_t l = 0; l < g.n_levels[p]; l++) {
            pf_level_args a{};
            a.m.pair_ref = pair_ref, a.m.w = g.lw[p][l], a.m.h = g.lh[p][l], a.m.level = l, a.m.first = 0;
            a.m.c1 = (0.01 * maxv) * (0.01 * maxv), a.m.c2 = (0.03 * maxv) * (0.03 * maxv);
            a.tab = tab, a.pyr = cur, a.out = nullptr, a.n_refs = g.n_refs, a.plane = p, a.maxv = g.maxv;
            const uint32_t tiles = l ? run_level<float>(a, g.n_pairs, out) : run_level<SAMPLE>(a, g.n_pairs, out);
            if (l == 0 && p == 0) tiles0 = tiles;
            if (l + 1 == g.n_levels[p]) break;
            pf_pool_args q{};
            q.tab = tab, q.src = cur, q.plane = p, q.maxv = g.maxv, q.w = g.lw[p][l], q.h = g.lh[p][l], q.ow = g.lw[p][l + 1], q.oh = g.lh[p][l + 1];
            q.dst = exact<float>((size_t)n_img * q.ow * q.oh);
            if (l) run_pool<float>(q, n_img);
            else run_pool<SAMPLE>(q, n_img);
            free(cur), cur = q.dst;
        }
        free(cur);
    }
    return tiles0;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned depth, w, h, sub, n_refs, n_pairs, levels;
    for (; fscanf(cfg, "%u %u %u %u %u %u %u", &depth, &w, &h, &sub, &n_refs, &n_pairs, &levels) == 7; cases++) {
        if ((depth != 8 && depth != 10 && depth != 12) || !w || !h || sub > 3 || !n_refs || !n_pairs || (levels != 0 && levels != 1 && levels != 5)) return 66;
        if (levels && (levels == 1 ? std::min(w, h) < 11 : std::min(w, h) <= 160)) return 66;
        geometry g{};
        g.n_refs = n_refs, g.n_pairs = n_pairs, g.n_planes = sub == 3 ? 1 : 3, g.bps = depth == 8 ? 1 : 2, g.maxv = (1u << depth) - 1u;
        const uint32_t cw = sub == 0 ? w : (w + 1) / 2, ch = sub == 2 ? (h + 1) / 2 : h;
        for (uint32_t p = 0; p < g.n_planes; p++) {
            uint32_t pw = p ? cw : w, ph = p ? ch : h;
            const uint32_t m = std::min(pw, ph);
            g.n_levels[p] = levels == 5 && m > 160 ? 5 : levels >= 1 && m >= 11 ? 1 : 0;
            for (uint32_t l = 0; l < std::max(g.n_levels[p], 1u); l++) g.lw[p][l] = pw, g.lh[p][l] = ph, pw = (pw + (pw & 1u)) / 2, ph = (ph + (ph & 1u)) / 2;
        }
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
                const size_t rows = s ? ch : h, row = (size_t)(s == 0 ? w : layout ? 2 * cw : cw) * g.bps;
                unsigned long long pt;
                if (fscanf(cfg, "%llu", &pt) != 1 || pt < row) return 66;
                const size_t len = (rows - 1) * pt + row;
                base[s] = exact<uint8_t>(len), pitch[s] = pt;
                if (fread(base[s], 1, len, in) != len) return 68;
                blocks.push_back(base[s]);
            }
            for (uint32_t p = 0; p < 3; p++) {
                pf_plane e{};
                if (p < g.n_planes) {
                    const unsigned s = layout && p == 2 ? 1 : p;
                    e.base = base[s] + (layout && p == 2 ? g.bps : 0), e.pitch = pitch[s], e.step = layout && p ? 2 : 1, e.shift = msb ? 16 - depth : 0;
                }
                tab[i * 3 + p] = e;
            }
        }
        long long *res = exact<long long>((size_t)n_pairs * kPfOut);
        memset(res, 0, sizeof(long long) * n_pairs * kPfOut);
        // which path the rows of the call take (the kernel's own test, on the addresses it will see)
        unsigned long wide = 0, scalar = 0;
        for (uint32_t i = 0; i < n_pairs; i++)
            for (uint32_t p = 0; p < g.n_planes; p++)
                for (uint32_t r = 0; r < g.lh[p][0]; r++) {
                    const pf_plane &x = tab[(size_t)pair_ref[i] * 3 + p], &y = tab[((size_t)n_refs + i) * 3 + p];
                    const bool ok = g.bps == 1 ? pf_wide_ok<1>(x.base + r * x.pitch, x.step, p) && pf_wide_ok<1>(y.base + r * y.pitch, y.step, p)
                                               : pf_wide_ok<2>(x.base + r * x.pitch, x.step, p) && pf_wide_ok<2>(y.base + r * y.pitch, y.step, p);
                    (ok ? wide : scalar)++;
                }
        uint32_t tiles = 0;
        if (g.bps == 1) run_sse<1>(g, tab, pair_ref, res), tiles = run_levels<uint8_t>(g, tab, pair_ref, res);
        else run_sse<2>(g, tab, pair_ref, res), tiles = run_levels<uint16_t>(g, tab, pair_ref, res);
        fwrite(res, sizeof(long long), (size_t)n_pairs * kPfOut, out);
        printf("case %d %lu %lu %u\n", cases, wide, scalar, tiles);
        for (uint8_t *b : blocks) free(b);
        free(res), free(tab), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
