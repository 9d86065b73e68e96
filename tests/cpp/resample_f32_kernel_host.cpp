// The device code of the float resampler (codec-eval_amd/csrc/resample_f32_kernel.h) compiled for the host, as
// resample_kernel_host.cpp does for the 8-bit one: the HIP keywords are defined away, blockIdx / threadIdx are plain
// variables that a loop sets, and every thread of every block of the grids that plan_resample - the launcher's own geometry
// - returns runs in turn: resample_f32_h_stage for all 256 threads, then resample_f32_h_body for all 256, as the barrier
// between them orders a block on the device.  Built with -fsanitize=address,undefined and -ffp-contract=off by
// tests/resample_f32_host.py.  Everything is a heap block of exactly its size: the source, the image between the passes, the
// tap tables (built by the product's ce_build_resample_table_f64, ce_tables.cpp linked in), the LDS stand-in (the dynamic
// LDS the launch would ask for, refilled with a sentinel before every block so that taps a previous block staged cannot
// stand in for ones this block did not; a null pointer on the global-table route) and the destination behind guard floats.
// A load or store outside any of them stops the run.
//
// usage: resample_f32_kernel_host CONFIGS IN OUT.  CONFIGS holds one job per line:
//   table n_in n_out filter          OUT receives ksize (u32) and the table, n_out * (1 + ksize) doubles
//   case w h out_w out_h n filter    IN holds the n source images (floats); OUT receives the horizontal table (as above) if
//                                    out_w != w, the vertical one if out_h != h, then the n output images
// and stdout one line per pass that ran: "pass JOB h|v tiles grid lds_bytes lds clamp", `lds` 1 when the taps were staged.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_on_host.h"

#include "resample_f32_kernel.h"

bool ce_build_resample_table_f64(uint32_t n_in, uint32_t n_out, int filter, std::vector<double> &table, uint32_t *ksize);  // ce_tables.cpp

static const unsigned char kLdsSentinel = 0x5a;  // as a first tap or a tap count: far outside any source row
static const float kGuard = -77777.0f;

// the table of one axis in a block of exactly its size, and into OUT
static double *build_table(uint32_t n_in, uint32_t n_out, int filter, uint32_t *ksize, FILE *out)
{
    std::vector<double> t;
    if (!ce_build_resample_table_f64(n_in, n_out, filter, t, ksize)) return nullptr;
    if (t.size() != (size_t)n_out * (1 + *ksize)) return nullptr;
    double *tab = static_cast<double *>(malloc(t.size() * sizeof(double)));
    if (!tab) return nullptr;
    memcpy(tab, t.data(), t.size() * sizeof(double));
    fwrite(ksize, 4, 1, out);
    fwrite(tab, sizeof(double), t.size(), out);
    return tab;
}

static void run_h(const pass_launch &p, const double *tab, uint32_t n_out, uint32_t ksize)
{
    double *lds = p.lds ? static_cast<double *>(malloc(p.lds_bytes)) : nullptr;
    if (p.lds && !lds) exit(70);
    for (uint32_t b = 0; b < p.grid; b++) {
        blockIdx.x = b;
        if (p.lds) {
            memset(lds, kLdsSentinel, p.lds_bytes);
            for (unsigned t = 0; t < kThreads; t++) {
                threadIdx.x = t;
                resample_f32_h_stage(find_place(p.g), tab, n_out, ksize, lds);
            }
        }
        for (unsigned t = 0; t < kThreads; t++) {
            threadIdx.x = t;
            if (p.lds) resample_f32_h_body<true>(p.g, find_place(p.g), tab, n_out, ksize, lds);
            else resample_f32_h_body<false>(p.g, find_place(p.g), tab, n_out, ksize, nullptr);
        }
    }
    free(lds);
}

static void run_v(const pass_launch &p, const double *tab, uint32_t n_out, uint32_t ksize)
{
    for (uint32_t b = 0; b < p.grid; b++) {
        blockIdx.x = b;
        for (unsigned t = 0; t < kThreads; t++) {
            threadIdx.x = t;
            resample_f32_v_body(p.g, tab, n_out, ksize);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) return 64;
    FILE *cfg = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!cfg || !in || !out) return 65;
    char kind[16];
    int jobs = 0;
    for (; fscanf(cfg, "%15s", kind) == 1; jobs++) {
        if (!strcmp(kind, "table")) {
            unsigned n_in, n_out, ksize;
            int filter;
            if (fscanf(cfg, "%u %u %d", &n_in, &n_out, &filter) != 3) return 66;
            double *tab = build_table(n_in, n_out, filter, &ksize, out);
            if (!tab) return 67;
            free(tab);
            continue;
        }
        if (strcmp(kind, "case")) return 66;
        unsigned w, h, ow, oh, n;
        int filter;
        if (fscanf(cfg, "%u %u %u %u %u %d", &w, &h, &ow, &oh, &n, &filter) != 6) return 66;
        const bool horiz = ow != w, vert = oh != h;
        if (!horiz && !vert) return 66;  // a byte copy: the caller's, no kernel runs
        const size_t src_img = (size_t)w * h * 3, mid_img = (size_t)ow * h * 3, dst_img = (size_t)ow * oh * 3;
        float *src = static_cast<float *>(malloc(n * src_img * sizeof(float)));
        if (!src || fread(src, sizeof(float), n * src_img, in) != n * src_img) return 68;
        float *mid = horiz && vert ? static_cast<float *>(malloc(n * mid_img * sizeof(float))) : nullptr;
        if (horiz && vert && !mid) return 69;
        for (size_t i = 0; mid && i < n * mid_img; i++) mid[i] = kGuard;
        const size_t guard = 4;
        float *slab = static_cast<float *>(malloc((guard + n * dst_img) * sizeof(float)));
        if (!slab) return 69;
        for (size_t i = 0; i < guard + n * dst_img; i++) slab[i] = kGuard;
        uint32_t ksize_h = 0, ksize_v = 0;
        double *tab_h = horiz ? build_table(w, ow, filter, &ksize_h, out) : nullptr;
        double *tab_v = vert ? build_table(h, oh, filter, &ksize_v, out) : nullptr;
        if ((horiz && !tab_h) || (vert && !tab_v)) return 67;
        resample_launch r;
        if (!plan_resample(src, src_img, slab + guard, dst_img, w, h, ow, oh, n, horiz, vert, ksize_h, mid, &r)) return 71;
        if (horiz) {
            run_h(r.h, tab_h, ow, ksize_h);
            printf("pass %d h %u %u %zu %d %d\n", jobs, r.h.g.tiles, r.h.grid, r.h.lds_bytes, (int)r.h.lds, (int)r.h.g.clamp);
        }
        if (vert) {
            run_v(r.v, tab_v, oh, ksize_v);
            printf("pass %d v %u %u %zu %d %d\n", jobs, r.v.g.tiles, r.v.grid, r.v.lds_bytes, (int)r.v.lds, (int)r.v.g.clamp);
        }
        for (size_t i = 0; i < guard; i++)
            if (slab[i] != kGuard) {
                fprintf(stderr, "job %d wrote in front of its destination\n", jobs);
                return 2;
            }
        fwrite(slab + guard, sizeof(float), n * dst_img, out);
        free(tab_h), free(tab_v), free(slab), free(mid), free(src);
    }
    fclose(cfg), fclose(in), fclose(out);
    printf("done %d\n", jobs);
    return 0;
}
