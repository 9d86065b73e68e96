// The device code of VIFp (codec-eval_amd/csrc/plane_vif_kernel.h, with plane_fidelity_kernel.h's planes and sample rule and
// ln_fixed.h) compiled for the host, as plane_hvs_kernel_host.cpp does for PSNR-HVS: the HIP keywords are defined away, blockIdx /
// threadIdx are plain variables that a loop sets, and every thread of every block of the launcher's own grids runs in turn -
// per scale the reduce kernel over (tiles, images x planes) for the references the pairs name and for the tests, then the
// stats kernel over (tiles, pairs x planes), both phase by phase as their two barriers order a block on the device: vif_stage
// for all 256 threads, then vif_columns for all 256, then vif_lane for all 256, and vif_reduce_stage / _columns / _rows alike.
// A thread block's two integers are added here as the kernel's reduction adds them.  Built with
// -fsanitize=address,undefined and -ffp-contract=off by
// tests/test_plane_vif_kernel_host_cpu.py.  Everything is a heap block of exactly its size: every plane (pitch padding between
// its rows only, none after the last row), the pyramid, and the LDS stand-ins, which are refilled with NaN before every block,
// as the pyramid is before every case.
//
// usage: plane_vif_kernel_host CONFIGS IN OUT.  CONFIGS holds one case per line:
//   depth w h subsampling n_refs n_pairs pair_ref[n_pairs] then per image (references, then tests): layout msb_aligned
//   pitch[stored planes]
// IN holds per case and image the stored planes, each (rows - 1) * pitch + row bytes long; OUT receives per case n_pairs x 24
// u64: [plane][scale][num, den].  stdout: one line "case N scale1_thread_blocks dead_thread_blocks idle_lanes" each - the
// thread blocks of the scale-1 stats grid, those of all grids that found no tile, and the lanes of live blocks without a
// position - then "done N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "plane_vif_kernel.h"

template <typename T>
static T *exact(size_t n)
{
    T *p = static_cast<T *>(malloc(n ? n * sizeof(T) : 1));
    if (!p) exit(70);
    return p;
}

struct counts {
    unsigned long scale1_blocks = 0, dead_blocks = 0, idle_lanes = 0;
};

template <int N, class SAMPLE>
static void stats(vif_args a, uint32_t n_pairs, unsigned long long *out, counts *c)
{
    using G = vif_geom<N>;
    using STAGE = vif_stage_t<SAMPLE>;
    STAGE *s_in = exact<STAGE>(2 * G::in_len);
    double *s_col = static_cast<double *>(aligned_alloc(16, sizeof(double) * kVifStreams * G::col_len));
    if (!s_col) exit(70);
    // plane_vif.hip: ce_yuv_plane_vif - the grid is sized for luma
    gridDim.x = ((a.w[0] - N + kVifTileW) / kVifTileW) * ((a.h[0] - N + kVifTileH) / kVifTileH), gridDim.y = n_pairs * a.n_planes;
    a.first = 0;
    if (a.scale == 0) c->scale1_blocks += (unsigned long)gridDim.x * gridDim.y;
    for (uint32_t by = 0; by < gridDim.y; by++)
        for (uint32_t bx = 0; bx < gridDim.x; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(s_in, 0xff, sizeof(STAGE) * 2 * G::in_len);
            memset(s_col, 0xff, sizeof(double) * kVifStreams * G::col_len);
            for (unsigned th = 0; th < kVifThreads; th++) threadIdx.x = th, vif_stage<N, SAMPLE>(a, s_in);
            for (unsigned th = 0; th < kVifThreads; th++) threadIdx.x = th, vif_columns<N>(a, s_in, s_col);
            unsigned long long t[2] = {0, 0};
            const vif_where o = vif_block<N>(a);
            for (unsigned th = 0; th < kVifThreads; th++) {
                threadIdx.x = th;
                unsigned long long q[2];
                vif_lane<N>(a, s_col, q);
                t[0] += q[0], t[1] += q[1];
                const uint32_t lx = (th % (kVifTileW / 2)) * 2, ly = th / (kVifTileW / 2);
                if (o.live && (o.x0 + lx >= o.vw || o.y0 + ly >= o.vh)) c->idle_lanes++;
            }
            if (!o.live) c->dead_blocks++;
            for (int m = 0; m < 2; m++) out[(size_t)o.pair * kVifOut + ((size_t)o.plane * kVifScales + a.scale) * 2 + m] += t[m];
        }
    free(s_in), free(s_col);
}

// images [first, first + count), as plane_vif.hip's reduce_run launches them
template <int N, class SAMPLE>
static void reduce(vif_reduce_args q, uint32_t first, uint32_t count, counts *c)
{
    using G = vif_reduce_geom<N>;
    using STAGE = vif_stage_t<SAMPLE>;
    STAGE *s_in = exact<STAGE>(G::in_len);
    double *s_col = exact<double>(G::col_len);
    gridDim.x = ((q.ow[0] + kVifReduceTile - 1) / kVifReduceTile) * ((q.oh[0] + kVifReduceTile - 1) / kVifReduceTile), gridDim.y = count * q.n_planes;
    q.first = first;
    for (uint32_t by = 0; by < gridDim.y; by++)
        for (uint32_t bx = 0; bx < gridDim.x; bx++) {
            blockIdx.x = bx, blockIdx.y = by;
            memset(s_in, 0xff, sizeof(STAGE) * G::in_len);
            memset(s_col, 0xff, sizeof(double) * G::col_len);
            for (unsigned th = 0; th < kVifThreads; th++) threadIdx.x = th, vif_reduce_stage<N, SAMPLE>(q, s_in);
            for (unsigned th = 0; th < kVifThreads; th++) threadIdx.x = th, vif_reduce_columns<N>(q, s_in, s_col);
            for (unsigned th = 0; th < kVifThreads; th++) threadIdx.x = th, vif_reduce_rows<N>(q, s_col);
            if (!vif_reduce_block(q).live) c->dead_blocks++;
        }
    free(s_in), free(s_col);
}

template <class SAMPLE>
static void run(const pf_plane *tab, const uint32_t *pair_ref, uint32_t n_refs, uint32_t n_pairs, uint32_t n_planes, uint32_t depth,
                const uint32_t pw[3], const uint32_t ph[3], unsigned long long *out, counts *c)
{
    const size_t n_img = (size_t)n_refs + n_pairs;
    uint32_t w[3][kVifScales] = {}, h[3][kVifScales] = {};
    size_t off[3][kVifScales] = {}, pyr_len = 0;
    for (uint32_t p = 0; p < n_planes; p++) {
        if (pw[p] < 41 || ph[p] < 41) continue;
        uint32_t cw = pw[p], chh = ph[p];
        for (int s = 0; s < kVifScales; s++) {
            if (s) {
                cw = (cw - vif_taps(s) + 2) / 2, chh = (chh - vif_taps(s) + 2) / 2;
                off[p][s] = pyr_len, pyr_len += n_img * cw * chh;
            }
            w[p][s] = cw, h[p][s] = chh;
        }
    }
    double *pyr = exact<double>(pyr_len);
    memset(pyr, 0xff, sizeof(double) * pyr_len);
    std::vector<bool> named(n_refs, false);
    for (uint32_t i = 0; i < n_pairs; i++) named[pair_ref[i]] = true;
    vif_args a{};
    a.tab = tab, a.pyr = pyr, a.pair_ref = pair_ref, a.out = nullptr, a.n_refs = n_refs, a.n_planes = n_planes;
    a.maxv = (1u << depth) - 1u, a.unit = 1.0 / (double)(1u << (depth - 8));
    for (uint32_t s = 0; s < (uint32_t)kVifScales; s++) {
        if (s) {
            vif_reduce_args q{};
            q.tab = tab, q.src = pyr, q.dst = pyr, q.n_planes = n_planes, q.maxv = a.maxv, q.unit = a.unit;
            for (uint32_t p = 0; p < n_planes; p++) {
                q.w[p] = w[p][s - 1], q.h[p] = h[p][s - 1], q.ow[p] = w[p][s], q.oh[p] = h[p][s];
                q.src_off[p] = off[p][s - 1], q.dst_off[p] = off[p][s];
            }
            for (uint32_t r = 0; r <= n_refs; r++) {
                if (r < n_refs && !named[r]) continue;
                const uint32_t first = r, count = r < n_refs ? 1 : n_pairs;  // each named reference, then the tests
                if (s == 1) reduce<9, SAMPLE>(q, first, count, c);
                else if (s == 2) reduce<5, double>(q, first, count, c);
                else reduce<3, double>(q, first, count, c);
            }
        }
        a.scale = s;
        for (uint32_t p = 0; p < n_planes; p++) a.w[p] = w[p][s], a.h[p] = h[p][s], a.off[p] = off[p][s];
        if (s == 0) stats<17, SAMPLE>(a, n_pairs, out, c);
        else if (s == 1) stats<9, double>(a, n_pairs, out, c);
        else if (s == 2) stats<5, double>(a, n_pairs, out, c);
        else stats<3, double>(a, n_pairs, out, c);
    }
    free(pyr);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    int cases = 0;
    unsigned depth, w, h, sub, n_refs, n_pairs;
    for (; fscanf(cfg, "%u %u %u %u %u %u", &depth, &w, &h, &sub, &n_refs, &n_pairs) == 6; cases++) {
        if ((depth != 8 && depth != 10 && depth != 12) || w < 41 || h < 41 || sub > 3 || !n_refs || !n_pairs) return 66;
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
        unsigned long long *res = exact<unsigned long long>((size_t)n_pairs * kVifOut);
        memset(res, 0, sizeof(unsigned long long) * n_pairs * kVifOut);
        const uint32_t pw[3] = {w, cw, cw}, ph[3] = {h, ch, ch};
        counts c;
        if (bps == 1) run<uint8_t>(tab, pair_ref, n_refs, n_pairs, n_planes, depth, pw, ph, res, &c);
        else run<uint16_t>(tab, pair_ref, n_refs, n_pairs, n_planes, depth, pw, ph, res, &c);
        fwrite(res, sizeof(unsigned long long), (size_t)n_pairs * kVifOut, out);
        printf("case %d %lu %lu %lu\n", cases, c.scale1_blocks, c.dead_blocks, c.idle_lanes);
        for (uint8_t *b : blocks) free(b);
        free(res), free(tab), free(pair_ref);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", cases);
    return 0;
}
